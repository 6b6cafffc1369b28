"""Numpy statements of the products with a symmetric matrix given as entries, for
the CPU and GPU tests: the term lists, mv and outer executed as the kernels are specified (every product
rounded in the value type, added one by one from +0), the mixed-precision refinement loop on the host, and
the cases both suites share.  Nothing here touches the GPU."""
import functools

import numpy as np

from assembly_ref import dense_user, duplicated

LONG_ROW = 64  # rows with more terms than this are summed by a whole wave


def kept_entries(n, rows, cols, triangle):
    """boolean mask of the entries that count, under the assembly's index rules (ValueError for the ones it
    refuses)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    for k, (i, j) in enumerate(zip(rows, cols)):
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError("entry %d out of range" % k)
        if i < j and triangle == "lower":
            raise ValueError("entry %d has row < col" % k)
    return rows >= cols


def row_terms(n, rows, cols, triangle="lower"):
    """(row_start [n + 1], entry [T], index [T], info): the terms of row i, in ascending entry index, are
    (k, cols[k]) for the kept entries with rows[k] == i and (k, rows[k]) for those with cols[k] == i and
    rows[k] != i -- one entry at a time, as the conventions state it"""
    keep = kept_entries(n, rows, cols, triangle)
    lists = [[] for _ in range(n)]
    for k in range(len(rows)):
        if not keep[k]:
            continue
        i, j = int(rows[k]), int(cols[k])
        lists[i].append((k, j))
        if i != j:
            lists[j].append((k, i))
    lens = np.array([len(t) for t in lists], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    flat = [t for row in lists for t in row]
    entry = np.array([t[0] for t in flat], dtype=np.int32)
    index = np.array([t[1] for t in flat], dtype=np.int32)
    info = {"nnz": len(rows), "kept": int(keep.sum()), "terms": len(flat), "max_row": int(lens.max()) if n else 0,
            "long_rows": int((lens > LONG_ROW).sum())}
    return start, entry, index, info


def mv_model(n, rows, cols, triangle, values, x, dtype):
    """out[i, j] = the terms of row i folded in list order from +0, s = s + values[k] * x[idx, j], both
    operations rounded in `dtype`; x [n] or [n, q]"""
    start, entry, index, _ = row_terms(n, rows, cols, triangle)
    v = np.asarray(values).astype(dtype)
    x = np.asarray(x).astype(dtype)
    x2 = x.reshape(n, -1)
    out = np.zeros_like(x2)
    for i in range(n):
        s = np.zeros(x2.shape[1], dtype=dtype)
        for t in range(start[i], start[i + 1]):
            p = (v[entry[t]] * x2[index[t]]).astype(dtype)
            s = (s + p).astype(dtype)
        out[i] = s
    return out.reshape(x.shape)


def outer_model(n, rows, cols, triangle, g, x, dtype):
    """out[k]: s = +0; for j ascending: t = g[r, j] * x[c, j]; if r != c: t = t + g[c, j] * x[r, j]; s = s + t;
    every operation rounded in `dtype`; 0 for a skipped entry"""
    keep = kept_entries(n, rows, cols, triangle)
    g2 = np.asarray(g).astype(dtype).reshape(n, -1)
    x2 = np.asarray(x).astype(dtype).reshape(n, -1)
    r, c = np.where(keep, rows, 0), np.where(keep, cols, 0)
    s = np.zeros(len(rows), dtype=dtype)
    for j in range(g2.shape[1]):
        t = (g2[r, j] * x2[c, j]).astype(dtype)
        u = (t + (g2[c, j] * x2[r, j]).astype(dtype)).astype(dtype)
        s = (s + np.where(r != c, u, t)).astype(dtype)
    return np.where(keep, s, dtype(0)).astype(dtype)


def dense_ld(n, rows, cols, values):
    """the matrix of the entries in np.longdouble, the kept ones summed at their position and mirrored"""
    keep = np.asarray(rows) >= np.asarray(cols)
    L = np.zeros((n, n), dtype=np.longdouble)
    np.add.at(L, (np.asarray(rows)[keep], np.asarray(cols)[keep]), np.asarray(values)[keep].astype(np.longdouble))
    return np.tril(L) + np.tril(L, -1).T


def abs_dense(n, rows, cols, values):
    """|A| of the bounds: the matrix of the entries' absolute values, so that (|A| |x|)_i is the sum of the
    absolute products of row i whatever cancels among duplicates"""
    return dense_user(n, np.asarray(rows), np.asarray(cols), np.abs(np.asarray(values, dtype=np.float64)))


def mv_bound(n, rows, cols, triangle, values, x, dtype):
    """(t_i + 1) eps (|A| |x|)_i per element: the bound of a sequential sum of t_i rounded products"""
    start = row_terms(n, rows, cols, triangle)[0]
    t = np.diff(start).astype(np.float64)
    ax = abs_dense(n, rows, cols, values) @ np.abs(np.asarray(x, dtype=np.float64)).reshape(n, -1)
    return ((t + 1)[:, None] * np.finfo(dtype).eps * ax).reshape(np.shape(x))


def outer_bound(n, rows, cols, g, x, dtype):
    """(2 q + 1) eps times the sum of the absolute products of every entry"""
    g2 = np.abs(np.asarray(g, dtype=np.float64)).reshape(n, -1)
    x2 = np.abs(np.asarray(x, dtype=np.float64)).reshape(n, -1)
    keep = np.asarray(rows) >= np.asarray(cols)
    r, c = np.where(keep, rows, 0), np.where(keep, cols, 0)
    tot = (g2[r] * x2[c]).sum(1) + np.where(r != c, (g2[c] * x2[r]).sum(1), 0.0)
    return (2 * g2.shape[1] + 1) * np.finfo(dtype).eps * tot


# ---- the cases ---------------------------------------------------------------------------------------
def _random_lower(n, rng, density):
    i, j = np.nonzero(np.tril(rng.random((n, n)) < density, -1))
    d = np.arange(n)
    return np.concatenate([d, i]).astype(np.int64), np.concatenate([d, j]).astype(np.int64)


def _arrow(t):
    """arrowhead of order t: the diagonal and the last row, whose list then has exactly t terms"""
    n = t
    d = np.arange(n)
    return n, np.concatenate([d, np.full(n - 1, n - 1)]).astype(np.int64), np.concatenate([d, d[:-1]]).astype(np.int64)


ARROWS = [63, 64, 65, 128, 129]
CASES = ["one", "empty", "gaps", "dups", "full", "blocks"] + ["arrow%d" % t for t in ARROWS]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(n, rows, cols, values (float64), triangle, param_sizes)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    sizes, triangle = None, "lower"
    if name == "one":
        n, rows, cols = 1, np.array([0]), np.array([0])
    elif name == "empty":
        n, rows, cols = 5, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    elif name == "gaps":  # rows 0, 1, 3, 4, 6 and 8 have no terms
        n, rows, cols = 9, np.array([2, 5, 7, 5, 7]), np.array([2, 2, 7, 5, 5])
    elif name in ("dups", "full"):
        n = 14
        r0, c0 = _random_lower(n, rng, 0.3)
        triangle = "full" if name == "full" else "lower"
        rows, cols, _ = duplicated(r0, c0, rng, max_dup=8, full=(name == "full"))
    elif name == "blocks":
        sizes = [2, 1, 4, 3, 1, 2, 4, 3]
        n = sum(sizes)
        rows, cols = _random_lower(n, rng, 0.25)
        order = rng.permutation(len(rows))
        rows, cols = rows[order], cols[order]
    elif name.startswith("arrow"):
        n, rows, cols = _arrow(int(name[5:]))
    else:
        raise KeyError(name)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return {"n": n, "rows": rows, "cols": cols, "values": rng.uniform(-1.0, 1.0, len(rows)), "triangle": triangle,
            "param_sizes": sizes}


@functools.lru_cache(maxsize=None)
def pattern(name):
    """the SymmetricPattern of a case (host work only)"""
    from baspacho_amd import sparse as S
    c = case(name)
    return S.SymmetricPattern(c["rows"], c["cols"], c["n"], param_sizes=c["param_sizes"], triangle=c["triangle"])


# ---- mixed-precision refinement ------------------------------------------------------------------------
GRIDS = {"g12_s0.1": (12, 0.1), "g20_s0.1": (20, 0.1), "g20_s0.01": (20, 0.01)}
GRID_COND = {"g12_s0.1": 37, "g20_s0.1": 56, "g20_s0.01": 146}
REFINE_ITERS = 3
REFINE_CAP = 1e-13  # no yardstick looser than this counts: a wrong loop cannot hide behind a bad one
REFINE_MARGIN = 8   # a kernel against its host model


def grid_entries(g, shift):
    """lower entries of the 5-point Laplacian of a g x g grid plus shift * I"""
    idx = np.arange(g * g).reshape(g, g)
    rows = np.concatenate([idx.ravel(), idx[:, 1:].ravel(), idx[1:, :].ravel()])
    cols = np.concatenate([idx.ravel(), idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    values = np.concatenate([np.full(g * g, 4.0 + shift), np.full(len(rows) - g * g, -1.0)])
    return g * g, rows.astype(np.int64), cols.astype(np.int64), values


def _chol_solve32(L, r):
    from scipy.linalg import solve_triangular
    y = solve_triangular(L, r.astype(np.float32), lower=True)
    return solve_triangular(L.T, y, lower=False).astype(np.float64)


def refine_model(A, b, iters):
    """solve_refined's loop on the host: a numpy fp32 Cholesky factor of A rounded to fp32, x = the fp32 solve
    of b, then `iters` times x += solve32(b - A x) with the residual in fp64"""
    L = np.linalg.cholesky(A.astype(np.float32))
    assert L.dtype == np.float32
    x = _chol_solve32(L, b)
    for _ in range(iters):
        x = x + _chol_solve32(L, b - A @ x)
    return x


def refine_reference(A, b):
    """A^-1 b refined with np.longdouble residuals until they stop mattering to float64"""
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    x = np.linalg.solve(A, b).astype(np.longdouble)
    for _ in range(4):
        x = x + np.linalg.solve(A, (bl - Al @ x).astype(np.float64)).astype(np.longdouble)
    return x


def rel_err(x, ref):
    """max |x - x_ref| / max |x_ref|"""
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(x).astype(np.longdouble) - ref)) / np.max(np.abs(ref)))


@functools.lru_cache(maxsize=None)
def refine_case(name):
    """a grid case with three right-hand sides: the entries, b [n, 3], the longdouble-refined reference, and
    the errors of the host model, of the float64 direct solve and of the plain fp32 solve against it"""
    g, shift = GRIDS[name]
    n, rows, cols, values = grid_entries(g, shift)
    A = dense_user(n, rows, cols, values)
    b = np.random.default_rng(g).uniform(-1.0, 1.0, (n, 3))
    ref = refine_reference(A, b)
    model = refine_model(A, b, REFINE_ITERS)
    L = np.linalg.cholesky(A.astype(np.float32))
    return {"n": n, "rows": rows, "cols": cols, "values": values, "A": A, "b": b, "ref": ref, "model": model,
            "cond": float(np.linalg.cond(A)), "model_err": rel_err(model, ref),
            "direct_err": rel_err(np.linalg.solve(A, b), ref), "fp32_err": rel_err(_chol_solve32(L, b), ref)}


def refine_bound(name):
    """what the GPU may miss the reference by: 8 x the host model's own error, capped"""
    return min(REFINE_MARGIN * refine_case(name)["model_err"], REFINE_CAP)
