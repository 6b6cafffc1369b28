"""Numpy restatement of the block diagonal of the reduced matrix S as preconditioner ("schur_jacobi", DESIGN.md
section 30), for the CPU and GPU tests: every table of the JacSchurJacobiPlan, the chunk partials, the blocks before
inversion and their inverses with the status record, in the summation orders the kernels are specified with
(hip_schur_kernels.h restates them), and the preconditioned reduced solve on top of schur_ref's model.  All block
arithmetic is float64 whatever the dtype of the values.  Nothing here touches the GPU."""
import functools

import numpy as np

import cg_ref as R
import schur_ref as SR

CHUNK = 64  # pairs of a chunk, rows of a pseudo-pair: part of the interface
MAX_BLOCK = 32


# ---- the tables ---------------------------------------------------------------------------------------------
def tables(case, eliminate):
    """every table of JacobianSchur.schurJacobiTable() for the Jacobian `case` with the params `eliminate` eliminated,
    and "widths": (w_b, w_e) of every pair"""
    rows, cols = np.asarray(case["rows"], dtype=np.int64), np.asarray(case["cols"], dtype=np.int64)
    m, n = case["m"], case["n"]
    sizes = np.ones(n, dtype=np.int64) if case["param_sizes"] is None else np.asarray(case["param_sizes"], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    param_of = np.repeat(np.arange(len(sizes)), sizes)
    elim = sorted(int(e) for e in eliminate)
    elim_index = {p: e for e, p in enumerate(elim)}
    kept = [p for p in range(len(sizes)) if p not in elim_index]
    kept_index = {p: b for b, p in enumerate(kept)}
    entry_at = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(rows, cols))}
    row_elim = np.full(m, -1, dtype=np.int64)
    touched = [set() for _ in range(m)]
    for i, j in zip(rows, cols):
        p = int(param_of[j])
        if p in elim_index:
            row_elim[i] = elim_index[p]
        else:
            touched[i].add(kept_index[p])
    free = len(elim)  # the free rows sort behind every eliminated param
    pair_rows = sorted((b, int(row_elim[i]) if row_elim[i] >= 0 else free, i) for i in range(m) for b in touched[i])
    t = {k: [] for k in ("pair_elim", "pair_row", "pair_rec", "row_of", "rec", "chunk_pair", "chunk_block", "widths")}
    block_pair = np.zeros(len(kept) + 1, dtype=np.int64)
    prev, in_pair = None, 0
    for x, (b, e, i) in enumerate(pair_rows):
        if prev != (b, e) or (e == free and in_pair == CHUNK):
            t["pair_elim"].append(-1 if e == free else e)
            t["pair_row"].append(x)
            t["pair_rec"].append(len(t["rec"]))
            t["widths"].append((int(sizes[kept[b]]), 0 if e == free else int(sizes[elim[e]])))
            block_pair[b + 1] += 1
            prev, in_pair = (b, e), 0
        in_pair += 1
        t["row_of"].append(i)
        scalars = list(range(start[kept[b]], start[kept[b] + 1]))
        if e != free:
            scalars += list(range(start[elim[e]], start[elim[e] + 1]))
        t["rec"].extend(entry_at.get((i, s), -1) for s in scalars)
    t["pair_row"].append(len(pair_rows))
    t["pair_rec"].append(len(t["rec"]))
    block_pair = np.cumsum(block_pair)
    widths = sizes[kept]
    block_chunk, chunk_part = [0], [0]
    for b in range(len(kept)):
        for p0 in range(block_pair[b], block_pair[b + 1], CHUNK):
            t["chunk_pair"].append(p0)
            t["chunk_block"].append(b)
            chunk_part.append(chunk_part[-1] + int(widths[b] * (widths[b] + 1) // 2))
        block_chunk.append(len(t["chunk_block"]))
    t["chunk_pair"].append(len(t["pair_elim"]))
    out = {k: np.asarray(v, dtype=np.int32) for k, v in t.items() if k != "widths"}
    out["widths"] = t["widths"]
    out["block_pair"], out["block_chunk"] = block_pair.astype(np.int32), np.asarray(block_chunk, dtype=np.int32)
    out["block_width"] = widths.astype(np.int32)
    out["block_off"] = np.concatenate([[0], np.cumsum(widths * widths)]).astype(np.int64)
    out["chunk_part"] = np.asarray(chunk_part, dtype=np.int64)
    out["kept_first"] = start[kept].astype(np.int64)
    return out


# ---- the sums -----------------------------------------------------------------------------------------------
def pair_sum(V, M, wb, binv):
    """W of one pair in float64 from its records' values V [rows, w_b + w_e] (present where M): G and F folded over
    the rows from +0, a term only where both entries exist; Y = Binv F and E = F^T Y folded over l ascending; W = G +
    (-E); a pseudo-pair (binv None): W = G.  Every product is rounded before it is added."""
    we = V.shape[1] - wb
    G, F = np.zeros((wb, wb)), np.zeros((we, wb))
    for v, mk in zip(V, M):
        has = mk[:wb, None] & mk[None, :wb]
        G[has] = (G + v[:wb, None] * v[None, :wb])[has]
        has = mk[wb:, None] & mk[None, :wb]
        F[has] = (F + v[wb:, None] * v[None, :wb])[has]
    if binv is None:
        return G
    Y = np.zeros((we, wb))
    for k in range(we):
        Y = Y + binv[:, k:k + 1] * F[k][None, :]
    E = np.zeros((wb, wb))
    for l in range(we):
        E = E + F[l][:, None] * Y[l][None, :]
    return G + (-E)


def build(t, values, binv, elim_off, d, dtype):
    """(minv, status, partials, blocks): the chunk partials (float64, lower triangles, element (a, c) at a (a + 1) / 2
    + c), the blocks A_b before inversion (lower triangle, float64, d added), their inverses as `dtype` at block_off
    and status = {the caller's scalar of the lowest bad pivot or -1, bad blocks}.  binv: the inverses of the
    eliminated blocks (schur_ref.Model.binv, with its block_off elim_off); d: the damping vector [n] or None"""
    v = np.asarray(values).astype(dtype).astype(np.float64)
    nb = len(t["block_width"])
    partials = np.zeros(int(t["chunk_part"][-1]))
    blocks = []
    with np.errstate(all="ignore"):
        for h, b in enumerate(t["chunk_block"]):
            wb = int(t["block_width"][b])
            P = np.zeros((wb, wb))
            for p in range(t["chunk_pair"][h], t["chunk_pair"][h + 1]):
                we = t["widths"][p][1]
                r0, r1 = t["pair_row"][p], t["pair_row"][p + 1]
                rec = t["rec"][t["pair_rec"][p]:t["pair_rec"][p + 1]].reshape(r1 - r0, wb + we)
                e = int(t["pair_elim"][p])
                bi = None if e < 0 else np.asarray(binv[elim_off[e]:elim_off[e + 1]]).astype(np.float64).reshape(we, we)
                P = P + pair_sum(np.where(rec >= 0, v[np.maximum(rec, 0)], 0.0), rec >= 0, wb, bi)
            partials[t["chunk_part"][h]:t["chunk_part"][h + 1]] = P[np.tril_indices(wb)]
        terms, tpos, tstart = [], [], [0]
        for b in range(nb):
            wb = int(t["block_width"][b])
            A = np.zeros((wb, wb))
            tril = np.tril_indices(wb)
            for h in range(t["block_chunk"][b], t["block_chunk"][b + 1]):
                Ph = np.zeros((wb, wb))
                Ph[tril] = partials[t["chunk_part"][h]:t["chunk_part"][h + 1]]
                A = A + Ph
            if d is not None:
                s0 = int(t["kept_first"][b])
                A[np.arange(wb), np.arange(wb)] += np.asarray(d[s0:s0 + wb]).astype(np.float64)
            blocks.append(np.tril(A))
            terms.extend(A[tril])
            tpos.extend(tril[0] * wb + tril[1])
            tstart.append(len(terms))
        compact = np.concatenate([[0], np.cumsum(t["block_width"])]).astype(np.int64)
        fake = (compact, np.asarray(tstart, dtype=np.int64), np.arange(len(terms)), np.asarray(tpos, dtype=np.int64))
        minv, off, status = R.build_block(fake, np.asarray(terms, dtype=np.float64), np.float64)
    assert np.array_equal(off, t["block_off"])
    if status[0] >= 0:  # compact kept index -> the caller's scalar
        b = int(np.searchsorted(compact, status[0], side="right")) - 1
        status[0] = int(t["kept_first"][b]) + int(status[0] - compact[b])
    return minv.astype(dtype), status, partials, blocks


class Precond:
    """ "schur_jacobi" on a schur_ref.Model: .minv, .status, .partials, .blocks and apply(r) (cg_ref.apply_block on the
    kept numbering)"""

    def __init__(self, mdl, t=None):
        self.t = t if t is not None else tables(mdl.case, _eliminated(mdl))
        self.minv, self.status, self.partials, self.blocks = build(self.t, mdl.v, mdl.binv, mdl.block_off, mdl.d, mdl.dt)
        self.compact = (np.concatenate([[0], np.cumsum(self.t["block_width"])]).astype(np.int64),)

    def apply(self, r):
        return R.apply_block(self.compact, self.minv, self.t["block_off"], r)


def _eliminated(mdl):
    return [int(p) for p in mdl.t["elim_param"]]


def dense_blocks(mdl, t):
    """per kept block (S_bb, bound_bb) in float64 from the dense J: the diagonal block of C - F^T B^-1 F and of |C| +
    |F|^T |B^-1| |F| (B^-1 the model's own inverses, so that a bad eliminated block drops out of both; |C| is the
    absolute value of the summed C, the tighter reading: the sum of the absolute terms |J_k|^T |J_k| is no smaller)"""
    cs = mdl.case
    import normal_eq_ref as N
    J = N.dense_j(mdl.m, mdl.n, cs["rows"], cs["cols"], mdl.v.astype(np.float64))
    ks, es = mdl.t["kept_scalar"], mdl.t["elim_scalar"]
    Jk, Je = J[:, ks], J[:, es]
    C, F = Jk.T @ Jk, Je.T @ Jk
    if mdl.d is not None:
        C = C + np.diag(mdl.d.astype(np.float64)[ks])
    Binv = np.zeros((len(es), len(es)))
    eo = mdl.t["elim_off"]
    for e in range(len(eo) - 1):
        w = eo[e + 1] - eo[e]
        Binv[eo[e]:eo[e + 1], eo[e]:eo[e + 1]] = mdl.binv[mdl.block_off[e]:mdl.block_off[e + 1]].reshape(w, w)
    S = C - F.T @ Binv @ F
    bound = np.abs(C) + np.abs(F).T @ np.abs(Binv) @ np.abs(F)
    c0 = np.concatenate([[0], np.cumsum(t["block_width"])])
    return [(S[c0[b]:c0[b + 1], c0[b]:c0[b + 1]], bound[c0[b]:c0[b + 1], c0[b]:c0[b + 1]]) for b in range(len(c0) - 1)]


# ---- the case of the chunk and pseudo-pair edges -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges_case():
    """(case, eliminate): 129 eliminated params (widths 1, 2, 3, 1, 2, 1, 8, 1 repeating; the last has zero values, so
    that its block of B is bad without damping) and nine kept ones:
      K0 width 32: 63 real pairs;  K1 width 1: 64;  K2 width 3: 65;  K3 width 2: 129 (the pair with eliminated param 0
      has 130 rows, the others 1);  K4 .. K7 width 2: 1, 64, 65 and 130 free rows and nothing else;  K8 width 2: no row
    Every eliminated param also has rows of its own entries alone (its block of B is well conditioned); some entries
    of K0 and of the wide eliminated params are left out (records with -1); the entries are shuffled."""
    rng = np.random.default_rng(30)
    ew = [(1, 2, 3, 1, 2, 1, 8, 1)[e % 8] for e in range(129)]
    sizes = ew + [32, 1, 3, 2, 2, 2, 2, 2, 2]
    K = list(range(129, 138))
    row_params = []
    for e in range(129):
        for k, upto in ((K[0], 63), (K[1], 64), (K[2], 65), (K[3], 129)):
            if e < upto:
                row_params.extend([(e, k)] * (130 if (e == 0 and k == K[3]) else 1))
        row_params.extend([(e,)] * (ew[e] + 1))
    for k, cnt in ((K[4], 1), (K[5], 64), (K[6], 65), (K[7], 130)):
        row_params.extend([(k,)] * cnt)
    c = SR._assemble(sizes, row_params, rng, identity=None, shuffle=False)
    start = np.concatenate([[0], np.cumsum(sizes)])
    first = np.zeros(c["n"], dtype=bool)
    first[start[:-1]] = True
    wide = np.zeros(c["n"], dtype=bool)  # scalars whose entries may be left out: never the first of a param
    wide[start[K[0]]:start[K[0] + 1]] = True
    for e in range(129):
        if ew[e] >= 2:
            wide[start[e]:start[e + 1]] = True
    drop = wide[c["cols"]] & ~first[c["cols"]] & (rng.uniform(size=len(c["cols"])) < 0.2)
    vals = c["values"].copy()
    vals[c["cols"] == start[128]] = 0.0  # the last eliminated param (width 1): B_e = 0
    order = rng.permutation(np.nonzero(~drop)[0])
    c = dict(c, rows=c["rows"][order], cols=c["cols"][order], values=vals[order])
    return c, tuple(range(129))


def case(name):
    return edges_case() if name == "edges" else SR.case(name)


CASES = ["ba", "w1", "w8", "hub", "edges"]
DAMPING = SR.DENSE_DAMPING

_OPERATORS = {}


def operator(name):
    """(case, eliminate, JacobianOperator, sparse.JacobianSchur) of the named case, built once per process"""
    if name != "edges":
        return SR.operator(name)
    from baspacho_amd import sparse as S
    if name not in _OPERATORS:
        c, elim = edges_case()
        jop = S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
        _OPERATORS[name] = (c, elim, jop, S.JacobianSchur(jop, np.asarray(elim, dtype=np.int64)))
    return _OPERATORS[name]


@functools.lru_cache(maxsize=None)
def plan(name):
    c, elim = case(name)
    return tables(c, elim)


@functools.lru_cache(maxsize=None)
def model(name, dtype, damped):
    """(schur_ref.Model, Precond) of the named case"""
    c, elim = case(name)
    mdl = SR.model(name, dtype, damped) if name != "edges" else SR.Model(c, elim, dtype,
                                                                         damping_ab=DAMPING if damped else None)
    return mdl, Precond(mdl, plan(name))
