"""CPU: the coordinate-entry assembly map without a GPU.  The C entry points
must be declared and exported; entryOffsets() must equal the pure-Python statement of assembly_ref.py
(blockOffset / flipped / the fold) on random structures with and without sparse-elimination ranges
and on explicit skeletons, in both triangle modes; the dense matrix of the offsets (host densify,
permuted back) must be the scipy matrix of the entries; errors must name the offending entry."""
import os
import re

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import _lib
from baspacho_amd import sparse as S
from assembly_ref import dense_user, duplicated, param_starts, ref_offsets, stored_elements
from helpers import solver_random
from selinv_cases import build_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bsp_assembly_create", "bsp_assembly_destroy", "bsp_assembly_entry_offsets", "bsp_assembly_info",
           "bsp_assemble_f64", "bsp_assemble_f32", "bsp_assemble_batched_f64", "bsp_assemble_batched_f32",
           "bsp_assemble_adjoint_f64", "bsp_assemble_adjoint_f32", "bsp_assemble_adjoint_batched_f64",
           "bsp_assemble_adjoint_batched_f32", "bsp_scalar_permutation"]


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % name, header), name
        assert hasattr(lib, name), name


def _structures():
    return [("random_elim", solver_random(71, size=18, fill=0.12, elim=(0, 8), ranges=[0, 8])[0]),
            ("random", solver_random(72, size=14, fill=0.15)[0]),
            ("random_wide", solver_random(73, size=30, fill=0.1, pmin=1, pmax=7)[0]),
            ("small/n3_r170", build_case("small/n3_r170")[0]),
            ("width17", build_case("width17")[0])]


STRUCTURES = _structures()


@pytest.mark.parametrize("name,sol", STRUCTURES, ids=[n for n, _ in STRUCTURES])
@pytest.mark.parametrize("triangle", ["lower", "full"])
def test_entry_offsets_match_reference(name, sol, triangle):
    rng = np.random.default_rng(len(name))
    r0, c0 = stored_elements(sol)
    rows, cols, values = duplicated(r0, c0, rng, full=(triangle == "full"))
    asm = sol.assembly(rows, cols, triangle)
    got = asm.entryOffsets()
    np.testing.assert_array_equal(got, ref_offsets(sol, rows, cols, triangle))
    if triangle == "full":
        assert np.all((got == -1) == (rows < cols))
    # every stored lower element is reached, and nothing else
    assert len(np.unique(got[got >= 0])) == len(r0)
    assert np.all(sol.lowerMask()[got[got >= 0]])
    # host assembly -> densify -> caller's order equals the scipy matrix of the entries
    data = np.zeros(sol.dataSize())
    keep = got >= 0
    np.add.at(data, got[keep], values[keep])
    sp = sol.scalarPermutation()
    dense = sol.densify(data, fill_upper_half=True)[np.ix_(sp, sp)]
    np.testing.assert_array_equal(dense, dense_user(sol.order(), rows, cols, values))
    info = asm.info()
    assert info["nnz"] == len(rows) and info["kept"] == int(keep.sum()) and info["elements"] == len(r0)
    assert info["max_run"] <= 8 and info["device_bytes"] > 0


def test_scalar_permutation():
    for _, sol in STRUCTURES:
        perm, ss = sol.paramToSpan(), sol.skel()["spanStart"]
        expect = np.concatenate([np.arange(ss[s], ss[s + 1]) for s in perm])
        np.testing.assert_array_equal(sol.scalarPermutation(), expect)
        assert sorted(sol.scalarPermutation()) == list(range(sol.order()))


def _missing_element(sol):
    """(row, col) in the caller's order, row > col, of an element outside the stored pattern"""
    mask = np.tril(sol.densify(np.ones(sol.dataSize())) != 0)
    a, b = np.nonzero(np.tril(~mask, -1))
    to_user = np.argsort(sol.scalarPermutation())
    i, j = to_user[a[0]], to_user[b[0]]
    return max(i, j), min(i, j)


def test_errors_name_the_entry():
    sol = STRUCTURES[0][1]
    n = sol.order()
    r0, c0 = stored_elements(sol)
    rows, cols = list(r0[:5]), list(c0[:5])
    with pytest.raises(RuntimeError, match=r"entry 3 at \(%d, 0\) is out of range" % n):
        sol.assembly(rows[:3] + [n] + rows[4:], cols[:3] + [0] + cols[4:])
    with pytest.raises(RuntimeError, match=r"entry 2 at \(0, -1\) is out of range"):
        sol.assembly(rows[:2] + [0], cols[:2] + [-1])
    i, j = _missing_element(sol)
    with pytest.raises(RuntimeError, match=r"entry 4 at \(%d, %d\) .*is not in the solver's stored pattern" % (i, j)):
        sol.assembly(rows[:4] + [i], cols[:4] + [j])
    k = int(np.nonzero(r0 != c0)[0][0])
    a, b = int(r0[k]), int(c0[k])
    with pytest.raises(RuntimeError, match=r"entry 1 at \(%d, %d\) has row < col" % (b, a)):
        sol.assembly([r0[1], b], [c0[1], a], "lower")
    # the same entry in full mode is skipped, not refused
    np.testing.assert_array_equal(sol.assembly([r0[1], b], [c0[1], a], "full").entryOffsets()[1:], [-1])
    with pytest.raises(ValueError, match="triangle"):
        sol.assembly(rows, cols, "upper")
    with pytest.raises(ValueError, match="rows for"):
        sol.assembly(rows, cols[:-1])


def test_nnz_zero():
    sol = STRUCTURES[1][1]
    asm = sol.assembly(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert asm.entryOffsets().shape == (0,)
    info = asm.info()
    assert info["nnz"] == 0 and info["kept"] == 0 and info["elements"] == 0
    assert info["tiles"] == (sol.dataSize() + 2047) // 2048


def test_long_runs_are_listed():
    sol = STRUCTURES[1][1]
    r0, c0 = stored_elements(sol)
    rows = np.concatenate([np.full(10001, r0[3]), r0])
    cols = np.concatenate([np.full(10001, c0[3]), c0])
    info = sol.assembly(rows, cols).info()
    assert info["max_run"] == 10002 and info["long_runs"] == 1


def test_assembly_keeps_its_solver():
    sol = solver_random(72, size=14, fill=0.15)[0]
    r0, c0 = stored_elements(sol)
    asm = sol.assembly(r0, c0)
    del sol
    assert asm.solver.dataSize() > 0
    assert len(asm.entryOffsets()) == len(r0)


def _scipy_block_structure(rows, cols, sizes):
    from scipy.sparse import coo_matrix
    starts = np.concatenate([[0], np.cumsum(sizes)])
    p = np.searchsorted(starts, rows, side="right") - 1
    q = np.searchsorted(starts, cols, side="right") - 1
    m = len(sizes)
    keep = p >= q
    A = coo_matrix((np.ones(int(keep.sum()) + m), (np.concatenate([p[keep], np.arange(m)]),
                                                    np.concatenate([q[keep], np.arange(m)]))), shape=(m, m)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr, A.indices


@pytest.mark.parametrize("sizes", [None, [2, 1, 3, 2, 1, 1, 2]])
@pytest.mark.parametrize("triangle", ["lower", "full"])
def test_symmetric_pattern_structure(sizes, triangle):
    rng = np.random.default_rng(5)
    n = 12
    ps = np.ones(n, dtype=np.int64) if sizes is None else np.asarray(sizes)
    i = rng.integers(0, n, size=60)
    j = rng.integers(0, n, size=60)
    rows, cols = (np.maximum(i, j), np.minimum(i, j)) if triangle == "lower" else (i, j)
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes, triangle=triangle)
    ptrs, inds = _scipy_block_structure(np.maximum(rows, cols) if triangle == "lower" else rows,
                                        np.minimum(rows, cols) if triangle == "lower" else cols, ps)
    np.testing.assert_array_equal(pat.structure.ptrs, ptrs)
    np.testing.assert_array_equal(pat.structure.inds, inds)
    np.testing.assert_array_equal(param_starts(pat.solver)[-1], n)
    got = pat.assembly.entryOffsets()
    np.testing.assert_array_equal(got, ref_offsets(pat.solver, rows, cols, triangle))


def test_symmetric_pattern_refuses_bad_entries():
    with pytest.raises(RuntimeError, match=r"entry 1 at \(0, 2\) has row < col"):
        S.SymmetricPattern([1, 0], [0, 2], 3)
    with pytest.raises(RuntimeError, match=r"entry 0 at \(5, 0\) is out of range"):
        S.SymmetricPattern([5], [0], 3)
    with pytest.raises(ValueError, match="param sizes"):
        S.SymmetricPattern([1], [0], 3, param_sizes=[1, 1])
