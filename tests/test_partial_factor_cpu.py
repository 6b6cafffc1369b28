"""The partial-factor checks of tests/known_factor.py can fail (no GPU needed).

factorUpTo(k) is simulated in numpy on the dense form of known-factor data of real solver structures:
a 64-wide blocked right-looking factor of the columns before the split (bar = spanStart[k]) whose
panels also update the trailing block (the cross-cut updates that form the Schur complement S).  It
runs once correctly (in the working precision) and once with one of the mistakes a plan or kernel
variant could make:
  P1  one cross-cut tile update dropped (the largest)
  P2  the cross-cut updates applied twice (a factorFrom that re-applies the sources before its start)
  P3  the cross-cut updates rounded through f32 (f64 only)
  P4  only the diagonal blocks of the trailing lumps updated
Every correct simulation must pass with a margin of 10 (the untouched trailing entries bitwise), every
mistake must fail by a factor of 10."""
import numpy as np
import pytest

from kf_structures import random_with_range
from known_factor import known_factor_data, ratios
from test_known_factor_cpu import LAZY, NB, STRUCTURES, _blocks, _fail_by, _pass_by

_cache = {}


# (the trailing blocks of width, grid and flat_schur hold no off-diagonal lump block that a cross-cut
#  update reaches at any split: P4 runs on a random structure with several dense lumps)
P4_STRUCTURES = [("random_with_range", lambda: random_with_range(7, LAZY))]


def _kf(name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        sol = dict(STRUCTURES + P4_STRUCTURES)[name]()
        _cache[key] = known_factor_data(sol, 29, dtype)
    return _cache[key]


def _split(sol):
    """the column of the split: the end of the elimination ranges when there are some, else the lump
    boundary nearest the middle"""
    ls = [int(x) for x in sol.skel()["lumpStart"]]
    er = [int(x) for x in sol.sparseEliminationRanges()]
    if er:
        return ls[er[-1]]
    inner = ls[1:-1]
    return min(inner, key=lambda c: abs(2 * c - ls[-1])) if inner else None


def _lump_of(sol):
    ls = sol.skel()["lumpStart"]
    return np.searchsorted(ls, np.arange(sol.order()), side="right") - 1


def blocked_partial(A, bar, dtype, drop=None, twice=False, update_dtype=None, lump_of=None):
    """factorUpTo in `dtype` arithmetic: 64-wide panels over the columns < bar, each updating the
    leading columns to its right and the trailing block (64 x 64 tiles from bar on).  drop=(k, i, j):
    the update of trailing tile (i, j) by panel k is skipped; twice: every cross-cut update is
    subtracted a second time; update_dtype: cross-cut update products rounded through that type;
    lump_of: cross-cut updates only land where row and column lie in the same lump"""
    M = np.array(A, dtype=dtype)
    n = len(M)
    lead, trail = _blocks(bar), [(b, min(b + NB, n)) for b in range(bar, n, NB)]
    for k, (k0, k1) in enumerate(lead):
        M[k0:k1, k0:k1] = np.linalg.cholesky(M[k0:k1, k0:k1])
        if k1 < n:
            M[k1:, k0:k1] = np.linalg.solve(M[k0:k1, k0:k1], M[k1:, k0:k1].T).T.astype(dtype)
        for i in range(k + 1, len(lead)):
            i0, i1 = lead[i]
            M[i0:, i0:i1] -= M[i0:, k0:k1] @ M[i0:i1, k0:k1].T
        for i, (i0, i1) in enumerate(trail):
            for j, (j0, j1) in enumerate(trail[:i + 1]):
                if drop == (k, i, j):
                    continue
                upd = M[i0:i1, k0:k1] @ M[j0:j1, k0:k1].T
                if update_dtype is not None:
                    upd = upd.astype(update_dtype).astype(dtype)
                if lump_of is not None:
                    upd = np.where(lump_of[i0:i1, None] == lump_of[None, j0:j1], upd, 0).astype(dtype)
                M[i0:i1, j0:j1] -= upd
                if twice:
                    M[i0:i1, j0:j1] -= upd
    return np.tril(M).astype(np.float64)


def _largest_cross_update(L, bar):
    """(k, i, j) of the cross-cut tile update with the largest norm"""
    n = len(L)
    lead, trail = _blocks(bar), [(b, min(b + NB, n)) for b in range(bar, n, NB)]
    best, arg = -1.0, None
    for k, (k0, k1) in enumerate(lead):
        for i, (i0, i1) in enumerate(trail):
            for j, (j0, j1) in enumerate(trail[:i + 1]):
                v = np.linalg.norm(L[i0:i1, k0:k1] @ L[j0:j1, k0:k1].T)
                if v > best:
                    best, arg = v, (k, i, j)
    return arg


def _ratios(kf, G, bar):
    return ratios(kf.partial_errors_dense(G, bar), kf.dtype)


def _names():
    """structures with a split: the width ones with a lump below the wide one, the grid, flat+Schur"""
    out = []
    for name, make in STRUCTURES:
        if _split(make()) is not None:
            out.append(name)
    return out


NAMES = _names()


def _cross_lump_split(kf):
    """the lump boundary below which cross-cut updates reach the most entries of off-diagonal lump
    blocks (the split where P4 differs most from a correct run)"""
    lo = _lump_of(kf.sol)
    best, arg = 0, None
    for bar in [int(x) for x in kf.sol.skel()["lumpStart"][1:-1]]:
        reach = ~kf.untouched(bar)[bar:, bar:] & kf.pattern[bar:, bar:]
        cnt = int(np.count_nonzero(reach & (lo[bar:, None] != lo[None, bar:])))
        if cnt > best:
            best, arg = cnt, bar
    return arg


def test_structures_have_splits():
    assert "grid" in NAMES and "flat_schur" in NAMES and any(n.startswith("width") for n in NAMES), NAMES


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_correct_partial_factor_passes(name, dtype):
    kf = _kf(name, dtype)
    bar = _split(kf.sol)
    G = blocked_partial(kf.A, bar, dtype)
    r = _ratios(kf, G, bar)
    assert _pass_by(r), (name, bar, r)
    # the entries no cross-cut product reaches keep their input bitwise
    mask = kf.untouched(bar)
    assert np.any(mask[bar:, bar:]) or name.startswith("width")
    assert np.array_equal(G[mask], np.tril(kf.A)[mask])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_dropped_cross_cut_update_fails(name, dtype):
    """P1"""
    kf = _kf(name, dtype)
    bar = _split(kf.sol)
    at = _largest_cross_update(kf.L, bar)
    r = _ratios(kf, blocked_partial(kf.A, bar, dtype, drop=at), bar)
    assert _fail_by(r), ("P1", name, at, r)
    assert r["schur"] >= 10.0 and max(r["lead_off"], r["lead_diag"], r["lead_backward"]) < 0.1, r


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_cross_cut_updates_applied_twice_fail(name, dtype):
    """P2"""
    kf = _kf(name, dtype)
    bar = _split(kf.sol)
    r = _ratios(kf, blocked_partial(kf.A, bar, dtype, twice=True), bar)
    assert _fail_by(r) and r["schur"] >= 10.0, ("P2", name, r)


@pytest.mark.parametrize("name", NAMES)
def test_cross_cut_updates_through_f32_fail(name):
    """P3"""
    kf = _kf(name, np.float64)
    bar = _split(kf.sol)
    r = _ratios(kf, blocked_partial(kf.A, bar, np.float64, update_dtype=np.float32), bar)
    assert _fail_by(r) and r["schur"] >= 10.0, ("P3", name, r)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", [n for n, _ in P4_STRUCTURES])
def test_diagonal_lump_blocks_only_fail(name, dtype):
    """P4, at the split where cross-cut updates reach off-diagonal lump blocks the most"""
    kf = _kf(name, dtype)
    bar = _cross_lump_split(kf)
    assert bar is not None
    r = _ratios(kf, blocked_partial(kf.A, bar, dtype), bar)
    assert _pass_by(r), (name, bar, r)
    r = _ratios(kf, blocked_partial(kf.A, bar, dtype, lump_of=_lump_of(kf.sol)), bar)
    assert _fail_by(r) and r["schur"] >= 10.0, ("P4", name, r)
