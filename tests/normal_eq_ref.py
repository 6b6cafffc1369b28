"""Pure-numpy statements of the normal equations of a sparse Jacobian, for the CPU
and GPU tests, and the Jacobians the tests run on.

Restatement: the pairs of every Jacobian row, their layout offsets through assembly_ref.ref_offsets, the
run order (ascending offset, ascending ka), H = np.add.at of the rounded products, the adjoint's term
listing, the column / row run sums of J^T r and J v, and the dense J in the caller's order."""
import numpy as np

from assembly_ref import ref_offsets

TILE, LONG_RUN = 2048, 64


def pair_offsets(sol, ca, cb):
    """layout offset of the stored lower element of every scalar pair (ca[k], cb[k]), ca >= cb: one
    ref_offsets call per distinct pair"""
    n = sol.order()
    key, inv = np.unique(np.asarray(ca, dtype=np.int64) * n + np.asarray(cb, dtype=np.int64), return_inverse=True)
    return ref_offsets(sol, key // n, key % n)[inv]


def row_groups(rows, m):
    """per Jacobian row, its entry indices in ascending order"""
    order = np.argsort(rows, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
    return [order[starts[i]:starts[i + 1]] for i in range(m)]


def ref_pair_table(sol, rows, cols, m):
    """(ka, kb, offset) in run order: every unordered pair of entries of a row, self-pairs included,
    cols[ka] >= cols[kb]; sorted by offset, then by ka"""
    ka, kb = [], []
    for ks in row_groups(rows, m):
        for x, a in enumerate(ks):
            for b in ks[:x + 1]:
                hi, lo = (a, b) if cols[a] >= cols[b] else (b, a)
                ka.append(hi)
                kb.append(lo)
    ka, kb = np.asarray(ka, dtype=np.int64), np.asarray(kb, dtype=np.int64)
    off = pair_offsets(sol, cols[ka], cols[kb]) if len(ka) else np.zeros(0, dtype=np.int64)
    order = np.lexsort((ka, off))
    return ka[order].astype(np.int32), kb[order].astype(np.int32), off[order]


def ref_hessian(sol, table, values, npdt):
    ka, kb, off = table
    v = values.astype(npdt)
    out = np.zeros(sol.dataSize(), dtype=npdt)
    np.add.at(out, off, v[ka] * v[kb])
    return out


def ref_adjoint_terms(sol, rows, cols, m):
    """(entry, partner, offset) of every adjoint term: per entry its row's entries in ascending index,
    itself twice in a row"""
    ent, par = [], []
    for ks in row_groups(rows, m):
        for k in ks:
            for p in ks:
                reps = 2 if p == k else 1
                ent.extend([k] * reps)
                par.extend([p] * reps)
    ent, par = np.asarray(ent, dtype=np.int64), np.asarray(par, dtype=np.int64)
    order = np.argsort(ent, kind="stable")
    ent, par = ent[order], par[order]
    off = pair_offsets(sol, np.maximum(cols[ent], cols[par]), np.minimum(cols[ent], cols[par])) if len(ent) \
        else np.zeros(0, dtype=np.int64)
    return ent, par, off


def ref_adjoint(terms, nnz, values, grad_data, npdt):
    ent, par, off = terms
    out = np.zeros(nnz, dtype=npdt)
    np.add.at(out, ent, grad_data.astype(npdt)[off] * values.astype(npdt)[par])
    return out


def ref_jt_vec(rows, cols, n, values, r, npdt):
    """g[c] = sum over the entries of column c, ascending k, of values[k] * r[rows[k]]"""
    r = r.astype(npdt)
    out = np.zeros((n,) + r.shape[1:], dtype=npdt)
    v = values.astype(npdt)
    np.add.at(out, cols, (v[:, None] * r[rows]) if r.ndim == 2 else v * r[rows])
    return out


def ref_j_vec(rows, cols, m, values, x, npdt):
    """y[i] = sum over the entries of row i, ascending k, of values[k] * x[cols[k]]"""
    x = x.astype(npdt)
    out = np.zeros((m,) + x.shape[1:], dtype=npdt)
    v = values.astype(npdt)
    np.add.at(out, rows, (v[:, None] * x[cols]) if x.ndim == 2 else v * x[cols])
    return out


def dense_j(m, n, rows, cols, values):
    J = np.zeros((m, n), dtype=np.float64)
    J[rows, cols] = values
    return J


def ref_info(sol, table, rows, cols, m):
    ka, kb, off = table
    nnz, P, n = len(rows), len(ka), sol.order()
    runs = np.unique(off, return_counts=True)[1] if P else np.zeros(0, dtype=np.int64)
    tiles = -(-sol.dataSize() // TILE)
    D, long_runs = len(runs), int((runs > LONG_RUN).sum())
    deg = np.bincount(rows, minlength=m)[rows] if nnz else np.zeros(0, dtype=np.int64)
    adj_long = int((deg + 1 > LONG_RUN).sum())
    return {"nnz": nnz, "pairs": P, "destinations": D, "max_run": int(runs.max()) if P else 0,
            "long_runs": long_runs, "tiles": tiles,
            "forward_bytes": 4 * (D + 1) + 8 * P + 8 * (tiles + 1) + 2 * D + 4 * long_runs,
            "adjoint_bytes": 8 * (nnz + 1) + 12 * 2 * P + 4 * adj_long,
            "vector_bytes": 4 * ((n + 1) + (m + 1) + 4 * nnz),
            "adjoint_terms": 2 * P}


# ---- Jacobians -------------------------------------------------------------------------------------
def _with_identity_rows(rows, cols, vals, m, n):
    """n more rows 2 e_i: J^T J >= 4 I"""
    rows = np.concatenate([np.asarray(rows, dtype=np.int64), m + np.arange(n)])
    cols = np.concatenate([np.asarray(cols, dtype=np.int64), np.arange(n)])
    return rows, cols, np.concatenate([vals, np.full(n, 2.0)]), m + n


def _rows_of_columns(col_sets, rng):
    rows = np.concatenate([np.full(len(c), i) for i, c in enumerate(col_sets)]).astype(np.int64)
    cols = np.concatenate([np.asarray(c) for c in col_sets]).astype(np.int64)
    return rows, cols, rng.uniform(-1, 1, len(rows))


def _shuffled(rows, cols, vals, rng):
    order = rng.permutation(len(rows))
    return rows[order], cols[order], vals[order]


def _case(rows, cols, vals, m, n, rng, param_sizes=None, keep=None, shuffle=True, identity=True):
    if identity:
        rows, cols, vals, m = _with_identity_rows(rows, cols, vals, m, n)
    if shuffle:
        rows, cols, vals = _shuffled(rows, cols, vals, rng)
    return {"rows": rows, "cols": cols, "values": vals, "m": m, "n": n, "param_sizes": param_sizes, "keep": keep}


def _scalar(rng, m=60, n=30):
    sets = [rng.choice(n, rng.integers(3, 6), replace=False) for _ in range(m)]
    return _case(*_rows_of_columns(sets, rng), m, n, rng)


def _blocks(rng, sizes, touching, m):
    """every residual row holds all the scalars of the params `touching(i)` gives it"""
    starts = np.concatenate([[0], np.cumsum(sizes)])
    sets = [np.concatenate([np.arange(starts[p], starts[p + 1]) for p in touching(i)]) for i in range(m)]
    return _rows_of_columns(sets, rng) + (m, int(starts[-1]))


def build(name):
    """dict(rows, cols, values, m, n, param_sizes, keep) of the named Jacobian"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "scalar":
        return _scalar(rng)
    if name == "scalar_small":  # for gradcheck
        return _scalar(rng, m=20, n=12)
    if name in ("blocks", "blocks_keep"):
        sizes = rng.integers(1, 8, 14)
        r, c, v, m, n = _blocks(rng, sizes, lambda i: rng.choice(14, rng.integers(2, 4), replace=False), 40)
        keep = None
        if name == "blocks_keep":
            starts = np.concatenate([[0], np.cumsum(sizes)])
            keep = rng.permutation(np.concatenate([np.arange(starts[p], starts[p + 1]) for p in (2, 7, 11)]))
        return _case(r, c, v, m, n, rng, param_sizes=sizes, keep=keep)
    if name == "blocks_elim":  # cameras and points: the points become an elimination range
        sizes = np.concatenate([rng.integers(5, 8, 5), np.full(60, 3)])
        r, c, v, m, n = _blocks(rng, sizes, lambda i: [int(rng.integers(0, 5)), 5 + i % 60], 180)
        return _case(r, c, v, m, n, rng, param_sizes=sizes)
    if name == "hub":
        # 300 rows on column 0 and on one of columns 1..3 (runs of 300 and of 100), one row of 70 entries
        n = 80
        sets = [np.array([0, 1 + i % 3, 4 + int(rng.integers(0, n - 4))]) for i in range(300)]
        sets.append(rng.permutation(n)[:70])
        return _case(*_rows_of_columns(sets, rng), len(sets), n, rng)
    if name == "longrun":
        sets = [np.array([3, 1])] * 12345
        return _case(*_rows_of_columns(sets, rng), len(sets), 5, rng)
    if name == "empty":
        return _case(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), 4, 3, rng, identity=False)
    if name == "empty_rows":
        c = _scalar(rng, m=20, n=10)
        c["rows"] = c["rows"] * 2 + 1  # every even row is empty; column 10 has one entry, in the last row
        c["m"], c["n"] = c["m"] * 2 + 3, 11
        c["rows"], c["cols"] = np.append(c["rows"], c["m"] - 1), np.append(c["cols"], 10)
        c["values"] = np.append(c["values"], 2.0)
        return c
    if name == "one":
        return _case(np.array([0]), np.array([0]), np.array([0.75]), 1, 1, rng, identity=False)
    if name == "tiles3":
        # one dense 72 x 72 block (5184 elements, three tiles), 70 dense rows: every lower element has a
        # run of 70 or 71 pairs, so each of the three tiles takes the wave path up to its boundary
        n = 72
        sets = [rng.permutation(n) for _ in range(70)]
        return _case(*_rows_of_columns(sets, rng), 70, n, rng, param_sizes=np.array([n]))
    raise KeyError(name)


CASES = ["scalar", "blocks", "blocks_keep", "blocks_elim", "hub", "longrun", "empty", "empty_rows", "one", "tiles3"]
_PATTERNS = {}


def pattern(name):
    """(case, JacobianPattern) of the named Jacobian, built once per process"""
    from baspacho_amd import sparse as S
    if name not in _PATTERNS:
        c = build(name)
        _PATTERNS[name] = (c, S.JacobianPattern(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"],
                                                keep=c["keep"]))
    return _PATTERNS[name]


_REFS = {}


def reference(name):
    """(pair table, adjoint terms) of the named Jacobian by the restatement, computed once per process"""
    if name not in _REFS:
        c, pat = pattern(name)
        _REFS[name] = (ref_pair_table(pat.solver, c["rows"], c["cols"], c["m"]),
                       ref_adjoint_terms(pat.solver, c["rows"], c["cols"], c["m"]))
    return _REFS[name]
