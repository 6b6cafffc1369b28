"""CPU: the factor status and the damping of the diagonal -- the symbols are
exported, bad arguments are refused before any device work, and the numpy restatement the GPU tests
compare against (tests/factor_status_ref.py) gives one clear answer on the planted inputs."""
import ctypes
import os
import re

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import _lib
import factor_status_ref as R
from helpers import solver_random, spd_data
from kf_structures import random_with_range
from stress_cases import width_solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["bsp_factor_status_", "bsp_damp_"]
NAMES = [op + mid + sfx for op in OPS for mid in ("", "batched_") for sfx in ("f64", "f32")]
FAKE = 0x1000  # never dereferenced: every call below is refused first


def test_the_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "baspacho_amd.h")).read()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(bsp_solver\* s," % n, hdr), n
        assert hasattr(lib, n), n
    for name in ("factorStatus", "readFactorStatus", "dampDiagonal", "factorRegularized"):
        assert callable(getattr(B.Solver, name)), name
    assert issubclass(B.FactorizationError, RuntimeError) and "FactorizationError" in B.__all__
    err = B.FactorizationError("broke", {"ok": False, "first": 3})
    assert err.status["first"] == 3 and str(err) == "broke"


def _ptrs(n, value=FAKE):
    return (ctypes.c_void_p * n)(*([value] * n))


def _refused(lib, rc, *words):
    assert rc != 0
    msg = lib.bsp_last_error().decode()
    assert all(w in msg for w in words), msg


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_bad_arguments_are_refused_before_any_device_work(sfx):
    lib = _lib.load()
    sol, _, _ = solver_random(57)
    h, ns = sol._h, sol.numSpans()
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    status, statusB = getattr(lib, "bsp_factor_status_" + sfx), getattr(lib, "bsp_factor_status_batched_" + sfx)
    damp, dampB = getattr(lib, "bsp_damp_" + sfx), getattr(lib, "bsp_damp_batched_" + sfx)
    # NULL pointers
    _refused(lib, status(h, None, i64(0), i64(ns), p(FAKE)), "factorStatus", "NULL")
    _refused(lib, status(h, p(FAKE), i64(0), i64(ns), None), "factorStatus", "NULL")
    _refused(lib, damp(h, None, i64(0), i64(ns), p(FAKE)), "dampDiagonal", "NULL")
    _refused(lib, damp(h, p(FAKE), i64(0), i64(ns), None), "dampDiagonal", "NULL")
    _refused(lib, statusB(h, None, i64(0), i64(ns), p(FAKE), ctypes.c_int32(2)), "factorStatus", "NULL")
    _refused(lib, statusB(h, _ptrs(2), i64(0), i64(ns), None, ctypes.c_int32(2)), "factorStatus", "NULL")
    _refused(lib, statusB(h, _ptrs(2, None), i64(0), i64(ns), p(FAKE), ctypes.c_int32(2)), "factorStatus", "NULL")
    _refused(lib, dampB(h, None, i64(0), i64(ns), p(FAKE), ctypes.c_int32(2)), "dampDiagonal", "NULL")
    _refused(lib, dampB(h, _ptrs(2), i64(0), i64(ns), None, ctypes.c_int32(2)), "dampDiagonal", "NULL")
    # an empty batch
    for batch in (0, -3):
        _refused(lib, statusB(h, _ptrs(1), i64(0), i64(ns), p(FAKE), ctypes.c_int32(batch)), "factorStatus", "empty")
        _refused(lib, dampB(h, _ptrs(1), i64(0), i64(ns), p(FAKE), ctypes.c_int32(batch)), "dampDiagonal", "empty")
    # a range outside 0 <= span_begin <= span_end <= numSpans
    for b, e in ((-1, ns), (0, ns + 1), (3, 2), (ns + 1, ns + 1)):
        _refused(lib, status(h, p(FAKE), i64(b), i64(e), p(FAKE)), "factorStatus", "range")
        _refused(lib, damp(h, p(FAKE), i64(b), i64(e), p(FAKE)), "dampDiagonal", "range")
        _refused(lib, statusB(h, _ptrs(2), i64(b), i64(e), p(FAKE), ctypes.c_int32(2)), "factorStatus", "range")
        two = (ctypes.c_void_p * 2)(FAKE, FAKE + 8 * sol.dataSize())
        _refused(lib, dampB(h, two, i64(b), i64(e), p(FAKE), ctypes.c_int32(2)), "dampDiagonal", "range")
    # in place: two members on one buffer
    _refused(lib, dampB(h, _ptrs(2), i64(0), i64(0), p(FAKE), ctypes.c_int32(2)), "dampDiagonal", "overlap")


def test_python_wrappers_check_the_range_first():
    sol, _, _ = solver_random(57)
    for b, e in ((-1, None), (0, sol.numSpans() + 1), (3, 2)):
        with pytest.raises(ValueError, match="span range"):
            sol.factorStatus(None, b, e)
        with pytest.raises(ValueError, match="span range"):
            sol.dampDiagonal(None, 0.0, 1.0, b, e)


def test_decoding_a_record_names_the_callers_parameter():
    import torch
    sol, ps, _ = solver_random(57)
    ss, p2s = sol.skel()["spanStart"], sol.paramToSpan()
    for param in (0, 7, len(ps) - 1):
        span = int(p2s[param])
        first = int(ss[span]) + int(ps[param]) - 1
        bits = np.array([0.25, 7.5]).view(np.int64)
        st = sol.readFactorStatus(torch.tensor([first, 2, bits[0], bits[1]], dtype=torch.int64))
        assert st == {"ok": False, "first": first, "param": param, "offsetInParam": int(ps[param]) - 1, "count": 2,
                      "minDiag": 0.25, "maxDiag": 7.5}
    empty = np.array([np.inf, 0.0]).view(np.int64)
    sts = sol.readFactorStatus(torch.tensor([[-1, 0, empty[0], empty[1]]] * 2, dtype=torch.int64))
    assert sts == [{"ok": True, "first": -1, "param": None, "offsetInParam": None, "count": 0,
                    "minDiag": np.inf, "maxDiag": 0.0}] * 2


def _planted_scalars(sol):
    """internal scalars to plant at: the first, the last, the first and last of a lump in the middle,
    one inside a sparse-elimination range when there is one, the middle of the widest lump, and both
    sides of the first 64-column panel boundary"""
    ls = sol.skel()["lumpStart"]
    n, mid = sol.order(), sol.numLumps() // 2
    widest = int(np.argmax(np.diff(ls)))
    ks = {0, n - 1, int(ls[mid]), int(ls[mid + 1]) - 1, int(ls[widest] + ls[widest + 1]) // 2, 63, 64}
    er = sol.sparseEliminationRanges()
    if len(er):
        ks.add(int(ls[int(er[-1]) // 2]))
    return sorted(ks)


@pytest.mark.parametrize("name", ["random_with_range", "width65_tail70"])
def test_the_restatement_has_one_clear_answer_on_planted_pivots(name):
    sol = random_with_range(5) if name == "random_with_range" else width_solver(65, 70)
    data = spd_data(sol, 11)
    diag = sol.diagOffsets()
    clean = R.nan_cholesky(sol.densify(data))
    assert R.first_failing_pivot(sol.densify(data)) == -1 and np.isfinite(clean).all()
    ks = _planted_scalars(sol)
    assert len(ks) >= 4
    for k in ks:
        planted = R.plant_negative(sol, data, k)
        dense = sol.densify(planted)
        assert dense[k, k] <= -1.0  # the pivot is <= A_kk < 0: never a near-zero tie
        assert R.first_failing_pivot(dense) == k
        L = R.nan_cholesky(dense)
        assert np.isfinite(L[:, :k]).all() and np.isnan(L[k, k])
        assert np.array_equal(L[:, :k], clean[:, :k])  # columns before k do not depend on A_kk
        factor = np.zeros_like(data)
        factor[diag] = np.diag(L)
        first, count, mn, mx = R.decode(R.scan(sol, factor))
        assert first == k and count >= 1
        if k > 0:
            assert mn > 0 and mn <= np.diag(L)[:k].min() and mx >= np.diag(L)[:k].max()
        # a range that ends before k is clean, one that starts behind k does not see k
        sp_of_k = int(np.searchsorted(sol.skel()["spanStart"], k, side="right")) - 1
        assert R.decode(R.scan(sol, factor, 0, sp_of_k))[:2] == (-1, 0)
        assert R.decode(R.scan(sol, factor, sp_of_k + 1, sol.numSpans()))[0] != k


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_of_scan_and_damp(dtype):
    sol, _, _ = solver_random(57)
    n, ns = sol.order(), sol.numSpans()
    data = spd_data(sol, 3, dtype=dtype)
    diag = sol.diagOffsets()
    assert R.decode(R.scan(sol, data)) == (-1, 0, float(data[diag].min()), float(data[diag].max()))
    assert R.decode(R.scan(sol, data, 4, 4)) == (-1, 0, np.inf, 0.0)  # an empty range
    tiny = np.finfo(dtype).smallest_subnormal
    for value, good in ((np.nan, False), (np.inf, False), (-np.inf, False), (0.0, False), (-0.0, False),
                        (-3.0, False), (tiny, True)):
        d = data.copy()
        d[diag[n - 1]] = value
        d[diag[5]] = value
        first, count, mn, mx = R.decode(R.scan(sol, d))
        assert (first, count) == ((-1, 0) if good else (5, 2)), value
        assert mn == (float(tiny) if good else float(np.delete(d[diag], [5, n - 1]).min()))
    # damp: the host Solver.damp in float64, three roundings in the data's type
    got = R.damp(sol, data, 0.125, 3.0)
    if dtype == np.float64:
        assert np.array_equal(got, sol.damp(data.copy(), 0.125, 3.0))
    a, b = dtype(1e-3), dtype(0.3)
    got = R.damp(sol, data, a, b, 2, ns - 1)
    ss = sol.skel()["spanStart"]
    idx = diag[int(ss[2]):int(ss[ns - 1])]
    want = data.copy()
    want[idx] = (want[idx] * dtype(dtype(1) + a)).astype(dtype) + b
    assert got.dtype == dtype and np.array_equal(got, want)
    rest = np.ones(len(data), dtype=bool)
    rest[idx] = False
    assert np.array_equal(got[rest], data[rest])
