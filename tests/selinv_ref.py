"""Reference and error metric of the selected-inversion tests.

Reference: Z_ref = inv(A) in fp64 of the densified input, A taken from the data as the kernel saw it
(an fp32 run is compared with the inverse of the fp32-rounded matrix, so input rounding is not
counted as kernel error).  For problems too large to invert densely, columns of A^-1 come from the
CPU oracle (cref.factor + cref.solve on unit vectors), independently of the library's solve().

Metric: every stored entry of the factor's layout (both triangles of the diagonal blocks included)
is compared in correlation units, |Z_got(i,j) - Z_ref(i,j)| / sqrt(Z_ref(i,i) Z_ref(j,j)).  For an
SPD matrix sqrt(Z_ii Z_jj) <= max|Z|, so this is never weaker than max|Z_got - Z_ref| / max|Z_ref|
and it sees the entries of weakly coupled blocks that a max-normalised error hides."""
import numpy as np

from oracle import cref


def stored_entries(sol):
    """(rows, cols, lump) of every element of the factor's data, rows and cols in span order"""
    sk = sol.skel()
    ls, ss = sk["lumpStart"], sk["spanStart"]
    rows = np.empty(sol.dataSize(), dtype=np.int64)
    cols = np.empty(sol.dataSize(), dtype=np.int64)
    lump = np.empty(sol.dataSize(), dtype=np.int64)
    cp, crs, cd = sk["chainColPtr"], sk["chainRowSpan"], sk["chainData"]
    for l in range(sol.numLumps()):
        c0, c1 = int(ls[l]), int(ls[l + 1])
        w = c1 - c0
        for c in range(int(cp[l]), int(cp[l + 1])):
            sp = int(crs[c])
            r0, r1 = int(ss[sp]), int(ss[sp + 1])
            d0 = int(cd[c])
            e = np.arange((r1 - r0) * w)
            rows[d0:d0 + len(e)] = r0 + e // w
            cols[d0:d0 + len(e)] = c0 + e % w
            lump[d0:d0 + len(e)] = l
    return rows, cols, lump


def pattern_of(sol, dense):
    """numeric data laid out by the skeleton, read from a dense (span order) matrix"""
    rows, cols, _ = stored_entries(sol)
    return dense[rows, cols]


def dense_reference(sol, data):
    """(A, inv(A)) in fp64 of the input `data` as stored (fp32 data: its rounded values), span order;
    the reference is checked: max|A X - I| is returned with it as the third value"""
    A = sol.densify(np.asarray(data).astype(np.float64), fill_upper_half=True)
    X = np.linalg.inv(A)
    X = 0.5 * (X + X.T)
    res = np.abs(A @ X - np.eye(len(A))).max()
    return A, X, res


def oracle_columns(sol, data, spans):
    """columns of A^-1 (span order) for every row of the given spans, from the CPU oracle's factor and
    solve: (column indices, X of shape (order, len(columns)))"""
    sk = sol.skel()
    L = np.ascontiguousarray(np.asarray(data), dtype=np.float64).copy()
    cref.factor(sk, L, sol.sparseEliminationRanges())
    ss = sk["spanStart"]
    idx = np.concatenate([np.arange(int(ss[s]), int(ss[s + 1])) for s in spans])
    n = sol.order()
    v = np.zeros(n * len(idx))
    v[idx + n * np.arange(len(idx))] = 1.0
    cref.solve(sk, L, v, n, len(idx))
    return idx, v.reshape(len(idx), n).T.copy()


class CorrError:
    """worst entry of the correlation-unit error, with where it sits"""

    def __init__(self, value, where):
        self.value, self.where = value, where

    def __repr__(self):
        return "%.3e at %s" % (self.value, self.where)


def _worst(err, rows, cols, lump):
    if len(err) == 0:
        return CorrError(0.0, "nothing stored")
    if not np.isfinite(err).all():
        i = int(np.argmax(~np.isfinite(err)))
        return CorrError(np.inf, "non-finite entry (%d, %d) of lump %d" % (rows[i], cols[i], lump[i]))
    i = int(np.argmax(err))
    return CorrError(float(err[i]), "entry (%d, %d) of lump %d" % (rows[i], cols[i], lump[i]))


def corr_error(sol, got, zref, entries=None):
    """worst |got - Z_ref| / sqrt(Z_ref(i,i) Z_ref(j,j)) over every stored entry; `got` is the
    selected inverse in the factor's layout, `zref` the dense reference inverse in span order"""
    rows, cols, lump = stored_entries(sol) if entries is None else entries
    d = np.diag(zref)
    assert (d > 0).all(), "the reference is not SPD"
    err = np.abs(np.asarray(got, dtype=np.float64) - zref[rows, cols]) / np.sqrt(d[rows] * d[cols])
    return _worst(err, rows, cols, lump)


def corr_error_columns(sol, got, idx, X, entries=None):
    """the metric on the stored entries whose column is one of `idx` (oracle_columns).  The diagonal
    of the reference is known for those columns only: a row outside them is normalised by the
    selected inverse's own diagonal entry (itself checked wherever its column is sampled)."""
    rows, cols, lump = stored_entries(sol) if entries is None else entries
    got = np.asarray(got, dtype=np.float64)
    pos = np.full(sol.order(), -1, dtype=np.int64)
    pos[idx] = np.arange(len(idx))
    sel = np.nonzero(pos[cols] >= 0)[0]
    r, c, lu = rows[sel], cols[sel], lump[sel]
    want = X[r, pos[c]]
    dref = X[idx, np.arange(len(idx))]
    dgot = got[np.nonzero(rows == cols)[0]]
    dg = np.empty(sol.order())
    dg[rows[rows == cols]] = dgot
    dr = np.where(pos[r] >= 0, dref[np.maximum(pos[r], 0)], dg[r])
    err = np.abs(got[sel] - want) / np.sqrt(dref[pos[c]] * np.abs(dr))
    return _worst(err, r, c, lu)


def max_normalised_error(sol, got, zref):
    """the former metric: max|got - Z_ref| / max|Z_ref| over the stored entries"""
    want = pattern_of(sol, zref)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


# ---- explicit skeletons -----------------------------------------------------------------------
def closed_skeleton(span_sizes, lump_to_span, below):
    """Solver.from_skeleton of a lump-column pattern closed under fill: `below[l]` lists span indices
    below lump l (any order); for each lump, every pair of its chain-row spans adds the lower span to
    the column of the upper span's lump (buildSelInvPlan needs the chain rows of a lump to form a
    clique)."""
    import baspacho_amd as B
    l2s = [int(x) for x in lump_to_span]
    nl = len(l2s) - 1
    span_lump = np.repeat(np.arange(nl), np.diff(l2s))
    rows = [set(int(s) for s in below.get(l, ())) for l in range(nl)]
    for l in range(nl):
        assert all(span_lump[s] > l for s in rows[l]), "rows below a lump must belong to later lumps"
        srt = sorted(rows[l])
        for i, a in enumerate(srt):
            la = span_lump[a]
            for b in srt[i + 1:]:
                if span_lump[b] != la:
                    rows[la].add(b)
    col_ptr, row_ind = [0], []
    for l in range(nl):
        row_ind += list(range(l2s[l], l2s[l + 1])) + sorted(rows[l])
        col_ptr.append(len(row_ind))
    span_start = np.concatenate([[0], np.cumsum(span_sizes)]).astype(np.int64)
    return B.Solver.from_skeleton(span_start, l2s, col_ptr, row_ind)


class SkelBuilder:
    """lumps appended one at a time (each a list of span sizes); below[l] filled by the caller"""

    def __init__(self):
        self.sizes, self.l2s, self.below = [], [0], {}

    def lump(self, span_sizes):
        self.sizes += [int(s) for s in span_sizes]
        self.l2s.append(len(self.sizes))
        return len(self.l2s) - 2

    def spans(self, lump):
        return list(range(self.l2s[lump], self.l2s[lump + 1]))

    def couple(self, lump, *others):
        """every span of the lumps `others` becomes a row below `lump`"""
        for o in others:
            self.below.setdefault(lump, set()).update(self.spans(o))

    def solver(self):
        return closed_skeleton(self.sizes, self.l2s, self.below)


def split_sizes(total, pattern):
    """span sizes summing to `total`, cycling through `pattern`"""
    out, i = [], 0
    while sum(out) < total:
        out.append(min(pattern[i % len(pattern)], total - sum(out)))
        i += 1
    return out


def lump_path(plan, lump):
    """("small", record) or ("node", [records right to left]) of one lump in a _testSelInvPlan()"""
    sm, nd = plan["small"], plan["node"]
    i = np.nonzero(sm["lump"] == lump)[0]
    if len(i):
        return "small", {f: int(v[i[0]]) for f, v in sm.items()}
    j = np.nonzero(nd["lump"] == lump)[0]
    return "node", [{f: int(v[k]) for f, v in nd.items()} for k in j]
