"""Pure-Python statements of the coordinate-entry assembly, for the CPU and GPU
tests: the entry -> layout offset map from blockOffset / flipped / the fold, the stored elements of a
solver in the caller's order, and entry sets with duplicates."""
import numpy as np


def param_starts(sol):
    """prefix sums of the param sizes in param order"""
    perm = sol.paramToSpan()
    ss = sol.skel()["spanStart"]
    return np.concatenate([[0], np.cumsum(ss[perm + 1] - ss[perm])]).astype(np.int64)


def ref_offsets(sol, rows, cols, triangle="lower"):
    """entry offsets as the conventions state them, one entry at a time (RuntimeError / ValueError as
    the library raises them is not restated: invalid entries raise ValueError here)"""
    perm = sol.paramToSpan()
    starts = param_starts(sol)
    n = sol.order()
    out = np.empty(len(rows), dtype=np.int64)
    for k, (i, j) in enumerate(zip(rows, cols)):
        i, j = int(i), int(j)
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError("entry %d out of range" % k)
        if i < j:
            if triangle == "lower":
                raise ValueError("entry %d has row < col" % k)
            out[k] = -1
            continue
        p = int(np.searchsorted(starts, i, side="right") - 1)
        q = int(np.searchsorted(starts, j, side="right") - 1)
        r, c = i - starts[p], j - starts[q]
        off, stride, flipped = sol.blockOffset(p, q)  # raises when the block is not stored
        if perm[p] == perm[q] and r < c:
            r, c = c, r
        out[k] = off + (c * stride + r if flipped else r * stride + c)
    return out


def stored_elements(sol):
    """(rows, cols) in the caller's order, row >= col, of every stored lower element of the factor"""
    mask = np.tril(sol.densify(np.ones(sol.dataSize())) != 0)
    a, b = np.nonzero(mask)  # internal order
    to_user = np.argsort(sol.scalarPermutation())
    i, j = to_user[a], to_user[b]
    return np.maximum(i, j).astype(np.int64), np.minimum(i, j).astype(np.int64)


def duplicated(rows, cols, rng, max_dup=8, full=False):
    """(rows, cols, values): every entry split into 1..max_dup contributions, shuffled; full: with
    mirrored (row < col) contributions besides"""
    reps = rng.integers(1, max_dup + 1, size=len(rows))
    r, c = np.repeat(rows, reps), np.repeat(cols, reps)
    if full:  # the mirror of about 30 % of the off-diagonal contributions, added (it is skipped)
        mirror = (rng.random(len(r)) < 0.3) & (r != c)
        r, c = np.concatenate([r, c[mirror]]), np.concatenate([c, r[mirror]])
    order = rng.permutation(len(r))
    return r[order], c[order], rng.uniform(-1.0, 1.0, size=len(r))


def dense_user(n, rows, cols, values):
    """the symmetric matrix the entries define: lower triangle summed, mirrored (scipy coo)"""
    from scipy.sparse import coo_matrix
    keep = rows >= cols
    L = coo_matrix((values[keep], (rows[keep], cols[keep])), shape=(n, n)).toarray()
    return np.tril(L) + np.tril(L, -1).T
