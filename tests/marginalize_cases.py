"""A random symmetric pattern in the caller's order for sparse.marginalize: params of mixed sizes,
full diagonal blocks, random off-diagonal blocks, duplicate entries, and a shuffled `keep` that covers
whole params."""
import numpy as np


def random_problem(seed, num_params=60, num_keep=9, fill=0.06, pmax=4):
    rng = np.random.default_rng(seed)
    ps = rng.integers(1, pmax + 1, size=num_params).astype(np.int64)
    n = int(ps.sum())
    st = np.concatenate([[0], np.cumsum(ps)])
    rows, cols = [], []
    for p in range(num_params):
        for i in range(st[p], st[p + 1]):
            for j in range(st[p], i + 1):
                rows.append(i)
                cols.append(j)
    for p in range(num_params):
        for q in range(p):
            if rng.random() < fill:
                for i in range(st[p], st[p + 1]):
                    for j in range(st[q], st[q + 1]):
                        rows.append(i)
                        cols.append(j)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    dup = rng.choice(len(rows), size=len(rows) // 5, replace=False)  # duplicates: their values add up
    rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
    order = rng.permutation(len(rows))
    rows, cols = rows[order], cols[order]
    kp = rng.choice(num_params, size=num_keep, replace=False)
    keep = np.concatenate([np.arange(st[p], st[p + 1]) for p in kp])
    rng.shuffle(keep)
    return {"rows": rows, "cols": cols, "n": n, "param_sizes": ps, "keep": keep, "keep_params": kp}


def spd_values(prob, seed, dtype=np.float64):
    """values of a well-conditioned SPD matrix on the entries (off-diagonal small, diagonal dominant)"""
    rng = np.random.default_rng(seed)
    rows, cols = prob["rows"], prob["cols"]
    v = rng.uniform(-1, 1, len(rows)) * 0.3
    v[rows == cols] = rng.uniform(4, 6, int((rows == cols).sum()))
    return v.astype(dtype)


def dense(prob, values):
    A = np.zeros((prob["n"], prob["n"]))
    np.add.at(A, (prob["rows"], prob["cols"]), np.asarray(values, dtype=np.float64))
    return np.tril(A) + np.tril(A, -1).T
