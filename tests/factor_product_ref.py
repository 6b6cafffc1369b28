"""Host reference of the products with the factor, y = L x and y = L^T x, shared by
tests/test_factor_product_cpu.py and tests/test_factor_product_gpu.py.

L is the lower triangle of the dense matrix of a buffer in the solver's layout (Solver.densify; the
strictly-upper elements of the diagonal blocks are not part of it).  The reference sums the stored elements
of every row (column, for the transpose) in np.longdouble for fp64 data and in float64 for fp32 data, and
reports with every output i

  t_i  the number of stored elements in its sum (stored: part of the block pattern, zero or not)
  s_i  sum_j |L_ij| |x_j|

so that the textbook bound of a length-t inner product in ANY summation order, with or without fma,

  |y_i - ref_i| <= t_i eps(dtype) s_i        (gamma_t = t u / (1 - t u) <= 2 t u = t eps)

is the acceptance test: no measured tolerance is involved.  Nothing here touches the GPU."""
import functools

import numpy as np

import baspacho_amd as B
from baspacho_amd import testing as T
import buffer_edges as E
import kf_structures as K
import selinv_cases


def stored_lower(sol):
    """boolean [n, n]: the positions i >= j that the layout stores (cached on the solver)"""
    got = getattr(sol, "_factor_product_stored", None)
    if got is None:
        got = np.tril(sol.densify(np.ones(sol.dataSize()))) != 0
        assert got.diagonal().all()
        sol._factor_product_stored = got
    return got


def dense_lower(sol, data):
    """tril of the dense matrix of `data` (host array in the layout) in float64; the strictly-upper elements
    of the diagonal blocks, whatever they hold, are left out"""
    return np.tril(sol.densify(E.clear_upper(np.asarray(data, dtype=np.float64), sol)))


def reference(sol, data, x, transposed):
    """(ref, t, s) for y = L x (or L^T x): ref [n, k] in the wide type, t [n] counts, s [n, k] float64.
    data: host array in the layout (float64 or float32), x: [n] or [n, k] of the same dtype"""
    data, x = np.asarray(data), np.asarray(x)
    assert data.dtype == x.dtype and data.dtype in (np.float64, np.float32)
    wide = np.longdouble if data.dtype == np.float64 else np.float64
    n = sol.order()
    x2 = x.reshape(n, -1)
    mask, Ld = stored_lower(sol), dense_lower(sol, data)
    if transposed:
        mask, Ld = mask.T, Ld.T
    rows, cols = np.nonzero(mask)  # row-major: ascending rows, every row present (the diagonal is stored)
    start = np.searchsorted(rows, np.arange(n))
    vals = Ld[rows, cols]
    ref = np.add.reduceat(vals.astype(wide)[:, None] * x2.astype(wide)[cols], start, axis=0)
    s = np.add.reduceat(np.abs(vals)[:, None] * np.abs(x2.astype(np.float64))[cols], start, axis=0)
    t = np.diff(np.append(start, len(rows)))
    return ref, t, s


def bound(t, s, dtype):
    """t_i eps s_i, [n, k]"""
    return t[:, None].astype(np.float64) * float(np.finfo(dtype).eps) * s


def check(sol, data, x, got, transposed, what=""):
    """asserts the element-wise bound of `got` ([n] or [n, k], the dtype of data) against the reference"""
    got = np.asarray(got)
    ref, t, s = reference(sol, data, x, transposed)
    g2 = got.reshape(ref.shape)
    assert np.isfinite(g2).all(), (what, "a result is not finite", int((~np.isfinite(g2)).sum()))
    err = np.abs(g2.astype(ref.dtype) - ref).astype(np.float64)
    lim = bound(t, s, data.dtype)
    bad = err > lim
    assert not bad.any(), (what, "outside t eps s", int(bad.sum()), np.argwhere(bad)[0].tolist(),
                           float(err[bad].max()), float(lim[bad].max()))


# ---- structures ------------------------------------------------------------------------------------------
def block_tridiagonal(num=30, size=9):
    """30 blocks of 9 scalars in a chain: five lumps of 36 to 117 columns after the supernode merge"""
    sizes = np.full(num, size, dtype=np.int64)
    cols = [[c] + ([c + 1] if c + 1 < num else []) for c in range(num)]
    st = B.Settings(findSparseEliminationRanges=False)
    return B.create_solver(st, sizes, T.columns_to_structure(cols), [])


def bal_small():
    """150 points of 3 scalars (one elimination range), 3 cameras of 9: every camera is seen by about 100
    points, so its row span collects more than 64 chains"""
    return K.bipartite(150, 3, 3, 9, seed=5, track=2)


def bal_huge():
    """1000 points of 3 scalars seen by one or both of 2 cameras of 9: a camera row sums the terms of more
    than 600 chains of 3 columns, then those of the 18-column camera lump"""
    return K.bipartite(1000, 2, 3, 9, seed=6, track=2)


EXTRA = {"tridiag": block_tridiagonal, "bal": bal_small, "bal_huge": bal_huge, "dense1": lambda: K.dense_solver(1),
         "dense64": lambda: K.dense_solver(64), "dense257": lambda: K.dense_solver(257),
         "bal_tall": lambda: K.bipartite(400, 1, 1, 70, seed=7, track=1)}


def structure_names():
    return selinv_cases.case_names() + list(EXTRA)


def build(name):
    """a NEW Solver of the named structure"""
    return EXTRA[name]() if name in EXTRA else selinv_cases.build_case(name)[0]


@functools.lru_cache(maxsize=None)
def solver(name):
    """the shared Solver of the named structure"""
    return build(name)


def random_operands(sol, dtype, k, seed):
    """(data with the sentinel in the strictly-upper diagonal-block elements, x [n, k]) in `dtype`"""
    rng = np.random.default_rng(seed)
    data = E.poison_upper(rng.uniform(-1.0, 1.0, sol.dataSize()).astype(dtype), sol)
    return data, rng.uniform(-1.0, 1.0, (sol.order(), k)).astype(dtype)


def counting_sort_plan(sk):
    """(spanChainPtr, spanChain, spanChainLump) of the skeleton dict: the chains sorted by row span, stable"""
    span = np.asarray(sk["chainRowSpan"], dtype=np.int64)
    nspans = len(sk["spanStart"]) - 1
    ptr = np.concatenate([[0], np.cumsum(np.bincount(span, minlength=nspans))])
    chains = np.argsort(span, kind="stable")
    lump = np.searchsorted(np.asarray(sk["chainColPtr"], dtype=np.int64), chains, side="right") - 1
    return ptr, chains, lump
