"""Numpy restatement of the factorised sparse approximate inverse preconditioner of DESIGN.md section 27
(kind 3, "fsai"), for the CPU and GPU tests: the host plan (pattern, items, column lists), the build of G row
by row in float64 scalars with every product rounded before it is added, the two ordered products of the
apply, and the whole preconditioned iteration through cg_ref.cg_model.  Also the generators of the matrices
the tests and the measurements use.  Nothing here touches the GPU."""
import functools
import math

import numpy as np

import cg_ref as R
from sym_product_ref import kept_entries

MAX_ROW = 32    # kCgFsaiMaxRow
LONG_RUN = 64   # kAssemblyLongRun: a longer column list is summed by a wave (the same sequential sum)
ITEM_LIMIT = 1 << 31


# ---- the plan -----------------------------------------------------------------------------------------------
def plan(n, rows, cols, triangle="lower"):
    """dict of int32 arrays.  S_i = cols[row_start[i] : row_start[i + 1]] ascending: the scalars j < i with a kept
    entry at (i, j) (whatever its value, duplicates once), the 31 largest when there are more, then i.  The items
    of row i, in ascending entry index k: the kept entries at (a, b), a >= b, both in S_i, with pos = la w + lb.
    Column j: (col_pos, col_row) of the elements of G in column j, rows ascending; long_cols: the columns of more
    than 64 terms."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    keep = kept_entries(n, rows, cols, triangle)
    before = [set() for _ in range(n)]
    for k in np.nonzero(keep)[0]:
        if rows[k] > cols[k]:
            before[rows[k]].add(int(cols[k]))
    S = [sorted(before[i])[-(MAX_ROW - 1):] + [i] for i in range(n)]
    row_start = np.concatenate([[0], np.cumsum([len(s) for s in S])]).astype(np.int64)
    local = [{a: l for l, a in enumerate(s)} for s in S]
    holders = [[] for _ in range(n)]          # C_a: the rows whose set holds a, ascending
    for i, s in enumerate(S):
        for a in s:
            holders[a].append(i)
    items = [[] for _ in range(n)]
    for k in np.nonzero(keep)[0]:
        a, b = int(rows[k]), int(cols[k])
        for i in holders[a]:
            if b in local[i]:
                items[i].append((int(k), local[i][a] * len(S[i]) + local[i][b]))
    count = sum(len(t) for t in items)
    check_sizes(int(row_start[-1]), count)
    col = [[(int(row_start[i]) + local[i][a], i) for i in holders[a]] for a in range(n)]
    col_start = np.concatenate([[0], np.cumsum([len(c) for c in col])])
    i32 = lambda a: np.array(a, dtype=np.int32).reshape(-1)
    flat = [t for row in items for t in row]
    cflat = [t for c in col for t in c]
    return {"row_start": i32(row_start), "cols": i32([a for s in S for a in s]),
            "item_start": i32(np.concatenate([[0], np.cumsum([len(t) for t in items])])),
            "entry": i32([t[0] for t in flat]), "pos": i32([t[1] for t in flat]),
            "col_start": i32(col_start), "col_pos": i32([t[0] for t in cflat]), "col_row": i32([t[1] for t in cflat]),
            "long_cols": i32([a for a in range(n) if len(col[a]) > LONG_RUN])}


def check_sizes(elems, items):
    """the plan's size check: both counts in [0, 2^31), the offending one stated"""
    for what, v in (("elements of G", elems), ("items", items)):
        if not 0 <= v < ITEM_LIMIT:
            raise ValueError("fsai has %d %s, outside [0, 2^31)" % (v, what))


# ---- the build ----------------------------------------------------------------------------------------------
def build(pl, values, dtype):
    """(G [elems] dtype, status [2] int64).  Row i, in float64 scalars, every product rounded before it is
    added: the local lower triangle summed from +0 in ascending entry index; Cholesky column by column (s =
    sqrt(d), A_ik = A_ik / s, A_ic = A_ic + (-(A_ik A_ck)), cgBlockBuild's sequence); the last row of L^-1: g_{w-1}
    = 1 / L_{w-1,w-1}, g_c = -(sum_{k = c+1}^{w-1} L_kc g_k) / L_cc with k ascending from +0; stored as dtype.  A
    pivot at local step k that is not positive and finite: the row is zeros; status = {the lowest S_i[k] over the
    bad rows or -1, the number of bad rows}"""
    v = np.asarray(values).astype(dtype)
    rs, cols, its, entry, pos = pl["row_start"], pl["cols"], pl["item_start"], pl["entry"], pl["pos"]
    n = len(rs) - 1
    G = np.zeros(int(rs[-1]), dtype=dtype)
    first, count = -1, 0
    for i in range(n):
        w = int(rs[i + 1] - rs[i])
        A = [0.0] * (w * w)
        for t in range(its[i], its[i + 1]):
            A[pos[t]] = A[pos[t]] + float(v[entry[t]])
        bad = -1
        for k in range(w):
            d = A[k * w + k]
            if not (d > 0.0 and math.isfinite(d)):
                bad = k
                break
            s = math.sqrt(d)
            A[k * w + k] = s
            for r in range(k + 1, w):
                A[r * w + k] = A[r * w + k] / s
            for r in range(k + 1, w):
                for c in range(k + 1, r + 1):
                    A[r * w + c] = A[r * w + c] + (-(A[r * w + k] * A[c * w + k]))
        if bad >= 0:
            count += 1
            scalar = int(cols[rs[i] + bad])
            first = scalar if first < 0 else min(first, scalar)
            continue
        g = [0.0] * w
        g[w - 1] = 1.0 / A[(w - 1) * w + (w - 1)]
        for c in range(w - 2, -1, -1):
            s = 0.0
            for k in range(c + 1, w):
                s = s + A[k * w + c] * g[k]
            g[c] = -s / A[c * w + c]
        G[rs[i]:rs[i + 1]] = np.array(g).astype(dtype)
    return G, np.array([first, count], dtype=np.int64)


def dense_rows(pl, A):
    """the independent evaluation: row i of G as the last row of the inverse of numpy.linalg.cholesky(A[S_i, S_i]),
    from the dense matrix A in np.longdouble where numpy's factorisation takes it (else float64)"""
    rs, cols = pl["row_start"], pl["cols"]
    out = np.zeros(int(rs[-1]), dtype=np.longdouble)
    for i in range(len(rs) - 1):
        s = cols[rs[i]:rs[i + 1]]
        L = _cholesky_ld(np.asarray(A, dtype=np.longdouble)[np.ix_(s, s)])
        w = len(s)
        g = np.zeros(w, dtype=np.longdouble)
        g[w - 1] = 1 / L[w - 1, w - 1]
        for c in range(w - 2, -1, -1):
            g[c] = -(L[c + 1:, c] @ g[c + 1:]) / L[c, c]
        out[rs[i]:rs[i + 1]] = g
    return out


def _cholesky_ld(M):
    """Cholesky in np.longdouble (numpy.linalg.cholesky refuses the type): the dot-product form, row by row"""
    w = M.shape[0]
    L = np.zeros_like(M)
    for r in range(w):
        for c in range(r):
            L[r, c] = (M[r, c] - L[r, :c] @ L[c, :c]) / L[c, c]
        L[r, r] = np.sqrt(M[r, r] - L[r, :r] @ L[r, :r])
    return L


# ---- the apply ----------------------------------------------------------------------------------------------
def apply(pl, G, r):
    """(t, z) for r [n, q] of G's dtype: t_i = dtype(sum_{j in S_i} float64(G_ij) float64(r_j)), j ascending from
    +0; z_j = dtype(sum_{i in C_j} float64(G_ij) float64(t_i)), i ascending from +0; every product rounded"""
    dt = r.dtype
    g64 = G.astype(np.float64)
    t = R.run_fold(pl["row_start"].astype(np.int64), g64[:, None] * r.astype(np.float64)[pl["cols"]], np.float64).astype(dt)
    z = R.run_fold(pl["col_start"].astype(np.int64), g64[pl["col_pos"]][:, None] * t.astype(np.float64)[pl["col_row"]],
                   np.float64).astype(dt)
    return t, z


def entries_model(n, rows, cols, values, b, dtype, triangle="lower", **kw):
    """cg_ref.cg_model on the matrix of the entries with the "fsai" preconditioner: (x, record, status)"""
    dt = np.dtype(dtype).type
    prod = R.Product(n, rows, cols, triangle)
    pl = plan(n, rows, cols, triangle)
    G, status = build(pl, values, dt)
    x, st = R.cg_model(n, lambda p: prod.mv(values, p, dt), b, dt, lambda r: apply(pl, G, r)[1], **kw)
    return x.reshape(np.shape(b)), st, status


# ---- the matrices -------------------------------------------------------------------------------------------
def ill_grid(gx, gy, bs, shift, seed=0, reach=1):
    """(n, rows, cols, values, sizes): lower entries of an ill-conditioned grid matrix.  gx x gy params of bs scalars;
    every pair of params within `reach` steps in both directions (8 neighbours for reach 1, 24 for reach 2) is an
    edge that adds Q = W^T W, W uniform in (0.2, 1), to both diagonal blocks and -Q to the block between them;
    `shift` times I is added at the end.  Fixed seed, one entry per position"""
    rng = np.random.default_rng(seed)
    n = gx * gy * bs
    A = np.zeros((n, n))
    idx = lambda x, y: (x * gy + y) * bs
    for x in range(gx):
        for y in range(gy):
            for dx in range(0, reach + 1):
                for dy in range(-reach, reach + 1):
                    if (dx, dy) <= (0, 0) or not (0 <= x + dx < gx and 0 <= y + dy < gy):
                        continue
                    W = rng.uniform(0.2, 1.0, (bs, bs))
                    Q = W.T @ W
                    p, q = idx(x, y), idx(x + dx, y + dy)
                    A[p:p + bs, p:p + bs] += Q
                    A[q:q + bs, q:q + bs] += Q
                    A[q:q + bs, p:p + bs] -= Q
                    A[p:p + bs, q:q + bs] -= Q.T
    A = (A + A.T) / 2 + shift * np.eye(n)
    i, j = np.nonzero(np.tril(A))
    return n, i.astype(np.int64), j.astype(np.int64), A[i, j].copy(), [bs] * (gx * gy)


@functools.lru_cache(maxsize=None)
def grid12():
    """the 12 x 12 grid of 3-wide params with shift 1e-3 (order 432, kappa_2 about 4e4)"""
    return ill_grid(12, 12, 3, 1e-3, seed=0)


def banded(n, half=33, seed=1):
    """lower entries of a diagonally dominant band matrix of half-bandwidth `half`: row i has min(i, half) entries
    before its diagonal, so the rows of G take every width 1 .. 32 and are then truncated to the 31 nearest"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n):
        for j in range(max(0, i - half), i):
            rows.append(i), cols.append(j), vals.append(rng.uniform(-1, 1))
        rows.append(i), cols.append(i), vals.append(2.0 * half + rng.uniform(1, 2))
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals)


def hub(later, n=70, seed=2):
    """(n, rows, cols, values): scalar 0 is a hub with entries (i, 0) to the `later` rows 1 .. later, so that column
    0 of G has later + 1 terms (its own row included): 63 later rows put it just at the long-run threshold of 64
    terms, 64 and 65 over it; a chain (i, i - 1) from row 2 on and a dominant diagonal besides"""
    rng = np.random.default_rng(seed)
    rows = list(range(1, later + 1)) + list(range(2, n)) + list(range(n))
    cols = [0] * later + list(range(1, n - 1)) + list(range(n))
    vals = np.concatenate([rng.uniform(-1, 1, len(rows) - n), 70.0 + rng.uniform(0, 1, n)])
    return n, np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), vals
