"""The known-factor checks of tests/known_factor.py can fail (no GPU needed).

Blocked right-looking Cholesky factors and blocked triangular solves are simulated in numpy on the
dense form of known-factor data of real solver structures, once correctly (in the working precision)
and once with one of the mistakes a kernel variant could make:
  M1  one tile update dropped (a 64 x 64 tile; a 1-wide edge tile of a 65-wide lump)
  M2  an f64 factor whose updates are rounded through f32
  M3  one tile update landing one row off
  M4  a forward or backward solve that ignores one off-diagonal block
  M5  an f64 solve through diagonal-block inverses computed in f32
  M6  one right-hand side of a group of 16 left unsolved on one block
Every correct simulation must pass with a margin of 10, every mistake must fail by a factor of 10."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from known_factor import factor_errors_dense, known_factor_data, ratios, solve_errors, sparsify, stored_pattern
from stress_cases import width_solver

NB = 64
LAZY = {"lazy_plan": 1}


def _grid_solver():
    ss = T.gen_grid(14, 11, 0.6, 2, 3)
    sizes = np.random.default_rng(3).integers(1, 4, size=ss.order()).astype(np.int64)
    return B.create_solver(B.Settings(hipOptions=LAZY), sizes, ss, [])


def _flat_schur_solver():
    base = T.gen_flat(60, 0.1, 7)
    k = 150
    ss = T.add_schur_set(base, k, 0.1, 1007)
    sizes = np.full(ss.order(), 3, dtype=np.int64)
    return B.create_solver(B.Settings(hipOptions=LAZY), sizes, ss, [0, k])


STRUCTURES = [("width%d_tail%d" % (W, tail), (lambda W=W, tail=tail: width_solver(W, tail, LAZY)))
              for W in (63, 64, 65, 255, 256, 257) for tail in (0, 70)] + \
             [("grid", _grid_solver), ("flat_schur", _flat_schur_solver)]

_cache = {}


def _kf(name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        sol = dict(STRUCTURES)[name]()
        _cache[key] = known_factor_data(sol, 11, dtype)
    return _cache[key]


def _blocks(n):
    return [(b, min(b + NB, n)) for b in range(0, n, NB)]


def blocked_cholesky(A, dtype, drop=None, shift=None, update_dtype=None):
    """64-wide right-looking blocked Cholesky in `dtype` arithmetic.  drop=(k, i, j): the update of
    target tile (i, j) by panel k is skipped; shift=(k, i, j): it lands one row lower;
    update_dtype: every update product is rounded through that type"""
    M = np.array(A, dtype=dtype)
    bl = _blocks(len(M))
    for k, (k0, k1) in enumerate(bl):
        M[k0:k1, k0:k1] = np.linalg.cholesky(M[k0:k1, k0:k1])
        Lkk = M[k0:k1, k0:k1]
        if k1 < len(M):
            M[k1:, k0:k1] = np.linalg.solve(Lkk, M[k1:, k0:k1].T).T.astype(dtype)
        for i in range(k + 1, len(bl)):
            i0, i1 = bl[i]
            for j in range(k + 1, i + 1):
                j0, j1 = bl[j]
                if drop == (k, i, j):
                    continue
                upd = M[i0:i1, k0:k1] @ M[j0:j1, k0:k1].T
                if update_dtype is not None:
                    upd = upd.astype(update_dtype).astype(dtype)
                if shift == (k, i, j):
                    M[i0 + 1:i1 + 1, j0:j1] -= upd[:len(M) - i0 - 1]
                else:
                    M[i0:i1, j0:j1] -= upd
    return np.tril(M).astype(np.float64)


def blocked_solve(L, b, dtype, skip_fwd=None, skip_bwd=None, inv_dtype=None, unsolved=None):
    """forward then backward blocked substitution in `dtype`.  skip_fwd / skip_bwd=(i, k): the
    off-diagonal block L[i, k] is ignored in that pass; inv_dtype: diagonal blocks applied through
    inverses computed in that type; unsolved=(blk, q): right-hand side q is not solved on block blk
    of the forward pass"""
    L = np.asarray(L, dtype=dtype)
    x = np.array(b, dtype=dtype).reshape(len(L), -1)
    bl = _blocks(len(L))

    def diag_solve(Lkk, r, trans):
        T_ = Lkk.T if trans else Lkk
        if inv_dtype is not None:
            inv = np.linalg.inv(T_.astype(inv_dtype)).astype(dtype)
            return inv @ r
        return np.linalg.solve(T_, r).astype(dtype)

    for k, (k0, k1) in enumerate(bl):
        keep = x[k0:k1].copy()
        x[k0:k1] = diag_solve(L[k0:k1, k0:k1], x[k0:k1], False)
        if unsolved is not None and unsolved[0] == k:
            x[k0:k1, unsolved[1]] = keep[:, unsolved[1]]
        for i in range(k + 1, len(bl)):
            if skip_fwd == (i, k):
                continue
            i0, i1 = bl[i]
            x[i0:i1] -= L[i0:i1, k0:k1] @ x[k0:k1]
    for k in range(len(bl) - 1, -1, -1):
        k0, k1 = bl[k]
        for i in range(k + 1, len(bl)):
            if skip_bwd == (i, k):
                continue
            i0, i1 = bl[i]
            x[k0:k1] -= L[i0:i1, k0:k1].T @ x[i0:i1]
        x[k0:k1] = diag_solve(L[k0:k1, k0:k1], x[k0:k1], True)
    return x.astype(np.float64)


def _largest_update(L, full_only=True):
    """(k, i, j) of the tile update with the largest norm (tiles 64 x 64 when full_only)"""
    bl = _blocks(len(L))
    best, arg = -1.0, None
    for k, (k0, k1) in enumerate(bl):
        for i in range(k + 1, len(bl)):
            for j in range(k + 1, i + 1):
                (i0, i1), (j0, j1) = bl[i], bl[j]
                if full_only and (i1 - i0 != NB or j1 - j0 != NB or k1 - k0 != NB):
                    continue
                v = np.linalg.norm(L[i0:i1, k0:k1] @ L[j0:j1, k0:k1].T)
                if v > best:
                    best, arg = v, (k, i, j)
    return arg


def _largest_block(L):
    bl = _blocks(len(L))
    best, arg = -1.0, None
    for k, (k0, k1) in enumerate(bl):
        for i in range(k + 1, len(bl)):
            i0, i1 = bl[i]
            v = np.linalg.norm(L[i0:i1, k0:k1])
            if v > best:
                best, arg = v, (i, k)
    return arg


def _fail_by(r, margin=10.0):
    return max(r.values()) >= margin


def _pass_by(r, margin=10.0):
    return max(r.values()) * margin <= 1.0


def _factor_ratios(kf, G):
    return ratios(factor_errors_dense(G, kf.L, kf.A, kf.pattern), kf.dtype)


def _rhs(n, nrhs, dtype, seed=5):
    return np.random.default_rng(seed).standard_normal((n, nrhs)).astype(dtype).astype(np.float64)


NAMES = [s[0] for s in STRUCTURES]
ONE_PANEL = ("width63_tail0", "width64_tail0")  # (no update, no off-diagonal block)
MULTI_PANEL = [s for s in NAMES if s not in ONE_PANEL]
FULL_TILES = [s for s in MULTI_PANEL if s != "width65_tail0"]  # (a 64 x 64 tile updated by a full panel)


def test_sparsify_inverts_densify():
    sol = width_solver(65, 70, LAZY)
    data = np.random.default_rng(1).standard_normal(sol.dataSize())
    A = sol.densify(data, fill_upper_half=True)
    back = sparsify(sol, A)
    mask = sol.lowerMask()
    assert np.array_equal(back[mask], data[mask])
    assert np.array_equal(sol.densify(back, fill_upper_half=True), A)


def test_pattern_holds_elimination_fill():
    """L0 L0^T stays inside the stored pattern of a structure with an elimination range (the assert
    inside known_factor_data), and the reference factor has no entry outside it"""
    kf = _kf("flat_schur", np.float64)
    assert len(kf.sol.sparseEliminationRanges()) >= 2
    assert np.abs(kf.L[np.tril(~stored_pattern(kf.sol))]).max(initial=0.0) < 1e-14


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_correct_blocked_factor_and_solve_pass(name, dtype):
    kf = _kf(name, dtype)
    G = blocked_cholesky(kf.A, dtype)
    r = _factor_ratios(kf, G)
    assert _pass_by(r), (name, r)
    n = len(kf.A)
    b = _rhs(n, 16, dtype)
    x = blocked_solve(G, b, dtype)
    r = ratios(solve_errors(kf.A, b, x), dtype)
    assert _pass_by(r), (name, r)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", FULL_TILES)
def test_dropped_tile_update_fails(name, dtype):
    """M1 (64 x 64 tile) and M3 (one row off) on the largest full-tile update of the factor"""
    kf = _kf(name, dtype)
    at = _largest_update(kf.L)
    r = _factor_ratios(kf, blocked_cholesky(kf.A, dtype, drop=at))
    assert _fail_by(r), ("M1", name, at, r)
    r = _factor_ratios(kf, blocked_cholesky(kf.A, dtype, shift=at))
    assert _fail_by(r), ("M3", name, at, r)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tail", [0, 70])
def test_dropped_edge_tile_fails(dtype, tail):
    """M1 on the 1-wide edge tile of a 65-wide lump: the update of column 64 by the first panel"""
    kf = _kf("width65_tail%d" % tail, dtype)
    r = _factor_ratios(kf, blocked_cholesky(kf.A, dtype, drop=(0, 1, 1)))
    assert _fail_by(r), ("M1 edge", tail, r)


@pytest.mark.parametrize("name", MULTI_PANEL)
def test_f64_updates_through_f32_fail(name):
    """M2"""
    kf = _kf(name, np.float64)
    r = _factor_ratios(kf, blocked_cholesky(kf.A, np.float64, update_dtype=np.float32))
    assert _fail_by(r), ("M2", name, r)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_solve_mistakes_fail(name, dtype):
    """M4 (either pass), M5 (f64 only) and M6, on the reference factor rounded to `dtype`"""
    kf = _kf(name, dtype)
    n = len(kf.A)
    G = np.tril(kf.L.astype(dtype).astype(np.float64))
    b = _rhs(n, 16, dtype)
    at = _largest_block(kf.L)
    if name in MULTI_PANEL:
        for kw in ("skip_fwd", "skip_bwd"):
            r = ratios(solve_errors(kf.A, b, blocked_solve(G, b, dtype, **{kw: at})), dtype)
            assert _fail_by(r), ("M4", kw, name, at, r)
    if dtype == np.float64:
        r = ratios(solve_errors(kf.A, b, blocked_solve(G, b, dtype, inv_dtype=np.float32)), dtype)
        assert _fail_by(r), ("M5", name, r)
    blk = len(_blocks(n)) // 2
    r = ratios(solve_errors(kf.A, b, blocked_solve(G, b, dtype, unsolved=(blk, 7))), dtype)
    assert _fail_by(r), ("M6", name, r)
