"""Numpy restatement of the implicit Schur elimination of DESIGN.md section 29, for the CPU and GPU tests: every
table of the JacSchurMap, the build of the eliminated blocks, the product with S, the reduction, the
back-substitution and the whole reduced solve (cg_ref's iteration on S), in float64 and float32.  The sums run in
the orders the kernels are specified with (hip_schur_kernels.h restates them).  What the conjugate gradient and the
least squares share is cg_ref's and cgls_ref's.  Nothing here touches the GPU."""
import functools

import numpy as np

import cg_ref as R
import cgls_ref as C
import normal_eq_ref as N

MAX_ELIM_WIDTH = 8


# ---- the tables ---------------------------------------------------------------------------------------------
def tables(case, eliminate):
    """every list of JacobianSchur.table() for the Jacobian `case` with the params `eliminate` eliminated"""
    rows, cols = np.asarray(case["rows"], dtype=np.int64), np.asarray(case["cols"], dtype=np.int64)
    m, n = case["m"], case["n"]
    sizes = np.ones(n, dtype=np.int64) if case["param_sizes"] is None else np.asarray(case["param_sizes"], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    elim = sorted(int(e) for e in eliminate)
    is_elim = np.zeros(len(sizes), dtype=bool)
    is_elim[elim] = True
    param_of = np.repeat(np.arange(len(sizes)), sizes)
    scalar_elim = is_elim[param_of]
    kept_scalar = np.nonzero(~scalar_elim)[0]
    elim_scalar = np.nonzero(scalar_elim)[0]
    kept_index = np.full(n, -1, dtype=np.int64)
    kept_index[kept_scalar] = np.arange(len(kept_scalar))
    elim_index = np.full(n, -1, dtype=np.int64)
    elim_index[elim_scalar] = np.arange(len(elim_scalar))
    elim_of_param = np.full(len(sizes), -1, dtype=np.int64)
    elim_of_param[elim] = np.arange(len(elim))
    elim_off = np.concatenate([[0], np.cumsum(sizes[elim])]).astype(np.int32)
    k_all = np.arange(len(rows))
    kk, ke = k_all[~scalar_elim[cols]], k_all[scalar_elim[cols]]

    def runs(ks, keys, other, num):
        s, entry, index, longs = C.run_list(keys[ks], other[ks], num)
        return s, ks[entry].astype(np.int32), index, longs

    t = {"rows_kept": runs(kk, rows, kept_index[cols], m), "rows_elim": runs(ke, rows, elim_index[cols], m),
         "cols_elim": runs(ke, elim_index[cols], rows, len(elim_scalar)),
         "cols_kept": runs(kk, kept_index[cols], rows, len(kept_scalar))}
    t["kept_scalar"], t["elim_scalar"] = kept_scalar.astype(np.int32), elim_scalar.astype(np.int32)
    t["elim_off"], t["elim_param"] = elim_off, np.asarray(elim, dtype=np.int32)
    row_elim = np.full(m, -1, dtype=np.int64)
    row_elim[rows[ke]] = elim_of_param[param_of[cols[ke]]]
    grouped = np.nonzero(row_elim >= 0)[0]
    order = np.argsort(row_elim[grouped], kind="stable")
    t["group_row"] = grouped[order].astype(np.int32)
    t["group_start"] = np.concatenate([[0], np.cumsum(np.bincount(row_elim[grouped], minlength=len(elim)))]).astype(np.int32)
    t["free_rows"] = np.nonzero(row_elim < 0)[0].astype(np.int32)
    # the blocks of B (eliminated params) and of C (kept params): cgls_ref.block_plan's items, restricted to a subset
    def blocks(params):
        index = np.full(len(sizes), -1, dtype=np.int64)
        index[params] = np.arange(len(params))
        lists = [[] for _ in params]
        for ks in N.row_groups(rows, m):
            per = {}
            for k in ks:
                b = int(index[param_of[cols[k]]])
                if b >= 0:
                    per.setdefault(b, []).append(int(k))
            for e, es in per.items():
                s, w = int(start[params[e]]), int(sizes[params[e]])
                for x, a in enumerate(es):
                    for b in es[:x + 1]:
                        hi, lo = (a, b) if cols[a] >= cols[b] else (b, a)
                        lists[e].append((hi, lo, (int(cols[hi]) - s) * w + (int(cols[lo]) - s)))
        flat = [x for e in lists for x in e]
        col = lambda i: np.array([x[i] for x in flat], dtype=np.int32)
        return (np.concatenate([start[params], [n]]).astype(np.int32), sizes[params].astype(np.int32),
                np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32), col(0), col(1), col(2))

    t["block_start"], t["block_width"], t["item_start"], t["item_a"], t["item_b"], t["item_pos"] = blocks(elim)
    kept_params = [p for p in range(len(sizes)) if not is_elim[p]]
    t["_kept_blocks"] = (lambda: blocks(kept_params), np.asarray(kept_params, dtype=np.int32))  # (built on demand)
    return t


def row_conflict(case, eliminate):
    """(row, param a, param b), a < b, of the lowest row with entries in two eliminated params, or None"""
    sizes = np.ones(case["n"], dtype=np.int64) if case["param_sizes"] is None else case["param_sizes"]
    param_of = np.repeat(np.arange(len(sizes)), sizes)
    elim = set(int(e) for e in eliminate)
    for i, ks in enumerate(N.row_groups(np.asarray(case["rows"], dtype=np.int64), case["m"])):
        seen = None
        for k in ks:
            p = int(param_of[case["cols"][k]])
            if p in elim:
                if seen is not None and seen != p:
                    return i, min(seen, p), max(seen, p)
                seen = p
    return None


# ---- the pieces ---------------------------------------------------------------------------------------------
class Model:
    """the pieces on one Jacobian, one set of values and one damping vector, in `dtype`"""

    def __init__(self, case, eliminate, dtype, values=None, damping_ab=None, t=None):
        self.dt = dt = np.dtype(dtype).type
        self.case, self.m, self.n = case, case["m"], case["n"]
        self.t = tables(case, eliminate) if t is None else t
        self.v = np.asarray(case["values"] if values is None else values).astype(dt)
        self.nK, self.nE = len(self.t["kept_scalar"]), len(self.t["elim_scalar"])
        self.csq = C.colsq(case["cols"], self.n, self.v, dt)
        self.d = None if damping_ab is None else C.damping(self.csq, damping_ab[0], damping_ab[1], dt)
        self.binv, self.block_off, self.status = self.build()
        # the inverses zero-padded to 8 x 8, [params, 8, 8] (a padded term adds +0 to a sum that is never -0)
        w = self.t["block_width"].astype(np.int64)
        self.pad = np.zeros((len(w), MAX_ELIM_WIDTH, MAX_ELIM_WIDTH), dtype=dt)
        for e in range(len(w)):
            self.pad[e, :w[e], :w[e]] = self.binv[self.block_off[e]:self.block_off[e + 1]].reshape(w[e], w[e])
        self.slot = np.concatenate([e * MAX_ELIM_WIDTH + np.arange(w[e]) for e in range(len(w))]).astype(np.int64)

    def build(self, plan=None, scalars=None):
        """(binv, block_off, status): cgls_ref.build_block's sums on the blocks of `plan` (default: the eliminated
        ones; items in list order from +0 in float64, double(d) added to the diagonal last), cg_ref.build_block's
        factorisation and inverse.  scalars: the caller's scalar of every scalar of the blocks, for the status"""
        t, v = self.t, self.v.astype(np.float64)
        if plan is None:
            plan = tuple(t[k] for k in ("block_start", "block_width", "item_start", "item_a", "item_b", "item_pos"))
            scalars = t["elim_scalar"]
        bs, bw, ist, ia, ib, ipos = plan
        terms, tpos, tstart = [], [], [0]
        for e, (s, w) in enumerate(zip(bs[:-1], bw)):
            sl = slice(ist[e], ist[e + 1])
            terms.extend(v[ia[sl]] * v[ib[sl]])
            tpos.extend(ipos[sl])
            if self.d is not None:
                terms.extend(self.d[s:s + w].astype(np.float64))
                tpos.extend(a * w + a for a in range(w))
            tstart.append(len(terms))
        compact = np.concatenate([[0], np.cumsum(bw)]).astype(np.int64)
        fake = (compact, np.asarray(tstart, dtype=np.int64), np.arange(len(terms)), np.asarray(tpos, dtype=np.int64))
        binv, off, status = R.build_block(fake, np.asarray(terms, dtype=np.float64), np.float64)
        if status[0] >= 0:
            status[0] = scalars[status[0]]
        return binv.astype(self.dt), off, status

    def precond(self, kind):
        """(apply, status) of a built-in preconditioner of S on the kept scalars: "jacobi", cgls_ref.build_jacobi on the
        kept scalars' column norms and damping; "block_jacobi", build() on the kept params' blocks of C with cg_ref's
        block apply"""
        ks = self.t["kept_scalar"]
        if kind == "jacobi":
            inv, status = C.build_jacobi(self.csq[ks], None if self.d is None else self.d[ks], self.dt)
            if status[0] >= 0:
                status[0] = ks[status[0]]
            return (lambda r: R.apply_jacobi(inv, r)), status
        plan = self.t["_kept_blocks"][0]()
        minv, off, status = self.build(plan, ks)
        compact = (np.concatenate([[0], np.cumsum(plan[1])]).astype(np.int64),)
        return (lambda r: R.apply_block(compact, minv, off, r)), status

    def _fold(self, which, vec):
        start, entry, index, _ = self.t[which]
        terms = (self.v[entry][:, None] * vec[index]).astype(self.dt)
        return R.run_fold(start.astype(np.int64), terms, self.dt)

    def _binv_apply(self, u):
        """y_l = the fold from +0 over l' ascending inside the param of Binv[l, l'] u_l'"""
        q = u.shape[1]
        up = np.zeros((self.pad.shape[0] * MAX_ELIM_WIDTH, q), dtype=self.dt)
        up[self.slot] = u
        up = up.reshape(-1, MAX_ELIM_WIDTH, q)
        y = np.zeros_like(up)
        for k in range(MAX_ELIM_WIDTH):
            y = (y + (self.pad[:, :, k, None] * up[:, None, k, :]).astype(self.dt)).astype(self.dt)
        return y.reshape(-1, q)[self.slot]

    def mv_t(self, p):
        """(S p, t) for p [nK, q]"""
        a = self._fold("rows_kept", p)
        y = self._binv_apply(self._fold("cols_elim", a))
        t = (a + (-self._fold("rows_elim", y))).astype(self.dt)
        out = self._fold("cols_kept", t)
        if self.d is not None:
            out = (out + (self.d[self.t["kept_scalar"]][:, None] * p).astype(self.dt)).astype(self.dt)
        return out, t

    def mv(self, p):
        return self.mv_t(np.asarray(p).astype(self.dt).reshape(self.nK, -1))[0]

    def full_rhs(self, r, c):
        """g = J^T r + c, the normal product of section 28"""
        cs = self.case
        if r is None:
            return np.asarray(c).astype(self.dt).reshape(self.n, -1)
        r = np.asarray(r).astype(self.dt).reshape(self.m, -1)
        c = None if c is None else np.asarray(c).astype(self.dt).reshape(self.n, -1)
        return C.epilogue_normal(N.ref_jt_vec(cs["rows"], cs["cols"], self.n, self.v, r, self.dt), None, None, c)

    def reduce(self, g):
        g = np.asarray(g).astype(self.dt).reshape(self.n, -1)
        h = self._fold("rows_elim", self._binv_apply(g[self.t["elim_scalar"]]))
        return (g[self.t["kept_scalar"]] + (-self._fold("cols_kept", h))).astype(self.dt)

    def back(self, g, xk):
        g = np.asarray(g).astype(self.dt).reshape(self.n, -1)
        xk = np.asarray(xk).astype(self.dt).reshape(self.nK, -1)
        u = self._fold("cols_elim", self._fold("rows_kept", xk))
        x = np.zeros_like(g)
        x[self.t["elim_scalar"]] = self._binv_apply((g[self.t["elim_scalar"]] + (-u)).astype(self.dt))
        x[self.t["kept_scalar"]] = xk
        return x

    def solve(self, r=None, c=None, precond=None, tol=1e-10, max_steps=100, x0=None, steps=None):
        """the reduced solve: (x [n, q], record of cg_ref.cg_model on S x_k = b_k); precond None, a callable, or
        "jacobi" / "block_jacobi" (then the preconditioner's status is left in self.precond_status)"""
        if isinstance(precond, str):
            precond, self.precond_status = self.precond(precond)
        g = self.full_rhs(r, c)
        bk = self.reduce(g)
        xk0 = None if x0 is None else np.asarray(x0).astype(self.dt).reshape(self.n, -1)[self.t["kept_scalar"]]
        with np.errstate(all="ignore"):
            xk, st = R.cg_model(self.nK, self.mv, bk, self.dt, apply_m=precond, tol=tol, max_steps=max_steps, x0=xk0,
                                steps=steps)
            return self.back(g, xk), st

    def dense_s(self, values=None):
        """(S, N) in float64 from the dense J: the reduced matrix on the kept scalars and the full N"""
        cs = self.case
        J = N.dense_j(self.m, self.n, cs["rows"], cs["cols"], self.v.astype(np.float64))
        Nm = J.T @ J
        if self.d is not None:
            Nm = Nm + np.diag(self.d.astype(np.float64))
        ks, es = self.t["kept_scalar"], self.t["elim_scalar"]
        S = Nm[np.ix_(ks, ks)] - Nm[np.ix_(ks, es)] @ np.linalg.solve(Nm[np.ix_(es, es)], Nm[np.ix_(es, ks)])
        return S, Nm


# ---- the Jacobians --------------------------------------------------------------------------------------------
def _assemble(sizes, row_params, rng, identity=2.0, scale=1.0, shuffle=True, extra_rows=0):
    """rows holding every scalar of the params row_params[i] (values uniform in (-1, 1) times `scale`), then
    `extra_rows` empty rows, then (identity not None) one row `identity` e_i per scalar"""
    sizes = np.asarray(sizes, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    n = int(start[-1])
    rows, cols = [], []
    for i, ps in enumerate(row_params):
        for p in ps:
            cols.extend(range(start[p], start[p + 1]))
            rows.extend([i] * int(sizes[p]))
    vals = list(rng.uniform(-1, 1, len(rows)) * scale)
    m = len(row_params) + extra_rows
    if identity is not None:
        rows.extend(range(m, m + n))
        cols.extend(range(n))
        vals.extend([identity] * n)
        m += n
    rows, cols, vals = np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals)
    if shuffle:
        order = rng.permutation(len(rows))
        rows, cols, vals = rows[order], cols[order], vals[order]
    return {"rows": rows, "cols": cols, "values": vals, "m": m, "n": n, "param_sizes": sizes, "keep": None}


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, eliminate) by name.
    "ba":     bundle-adjustment like: 5 cameras of 9 scalars and 14 points of 3, interleaved in the caller's order;
              every observation is 2 rows on one camera and one point; the points are eliminated
    "w1":     eliminated params of 1 scalar, kept ones of 2
    "w8":     eliminated params of 8 scalars, kept ones of 3 and 1
    "tiny":   3 eliminated params of 1 scalar, 2 kept ones of 2, 6 rows and the identity rows
    "hub":    groups of 1, 63, 64, 65, 129, 256 and 257 rows, kept columns of 65 and 129 entries, an eliminated scalar
              of 65 entries, a row with eliminated entries only, one with kept entries only, an eliminated param
              without rows and an empty row
    "bidiag_<nK>": a bidiagonal kept part on nK scalars, every row also on one of 7 eliminated scalars"""
    rng = np.random.default_rng(sum(map(ord, name)) + 29)
    if name == "ba":
        kinds = "cpppcppcpppcppcpppp"  # 5 cameras, 14 points
        sizes = [9 if k == "c" else 3 for k in kinds]
        cams = [i for i, k in enumerate(kinds) if k == "c"]
        pts = [i for i, k in enumerate(kinds) if k == "p"]
        obs = [(c, p) for p in pts for c in rng.choice(cams, rng.integers(2, 4), replace=False)]
        row_params = [ps for ps in obs for _ in range(2)]
        return _assemble(sizes, row_params, rng, scale=0.5), tuple(pts)
    if name == "w1":
        sizes = [1, 2, 2, 1, 1, 2, 1, 2, 1, 1]
        elim = [i for i, w in enumerate(sizes) if w == 1]
        kept = [i for i, w in enumerate(sizes) if w == 2]
        row_params = [(int(rng.choice(elim)), int(rng.choice(kept))) for _ in range(30)]
        return _assemble(sizes, row_params, rng, scale=0.5), tuple(elim)
    if name == "tiny":  # for gradcheck: 3 eliminated scalars, 4 kept ones
        sizes = [1, 2, 1, 2, 1]
        row_params = [(0, 1), (2, 1), (2, 3), (4, 3), (0, 3), (4, 1)]
        return _assemble(sizes, row_params, rng, scale=0.5), (0, 2, 4)
    if name == "w8":
        sizes = [3, 8, 1, 8, 3, 8, 1]
        elim = [1, 3, 5]
        kept = [0, 2, 4, 6]
        row_params = [(int(rng.choice(elim)),) + tuple(int(k) for k in rng.choice(kept, 2, replace=False)) for _ in range(40)]
        return _assemble(sizes, row_params, rng, scale=0.3), tuple(elim)
    if name == "hub":
        # params 0 .. 7 eliminated (width 1, 2, 3, 1, 2, 1, 8, 1; param 7 has no rows), then 20 kept scalars
        groups = [1, 63, 64, 65, 129, 256, 257]
        sizes = [1, 2, 3, 1, 2, 1, 8, 1] + [1] * 20
        kept = list(range(8, 28))
        row_params = []
        for e, cnt in enumerate(groups):
            for x in range(cnt):
                row_params.append((e, kept[(x + e) % 18 + 2]))
        row_params[1] = (1,)  # a row of group 1 with eliminated entries only
        row_params += [(kept[0],)] * 65 + [(kept[1],)] * 129  # kept columns of 65 and 129 entries, kept entries only
        c = _assemble(sizes, row_params, rng, identity=None, extra_rows=1)
        return c, tuple(range(8))
    if name.startswith("bidiag_"):
        nK = int(name.split("_")[1])
        b = C.bidiagonal(nK + 1, nK)
        nE = 7
        rows = np.concatenate([b["rows"], np.arange(nK + 1)])
        cols = np.concatenate([b["cols"] + nE, np.arange(nK + 1) % nE])
        vals = np.concatenate([b["values"], rng.uniform(0.5, 1.0, nK + 1)])
        order = rng.permutation(len(rows))
        c = {"rows": rows[order], "cols": cols[order], "values": vals[order], "m": nK + 1, "n": nK + nE,
             "param_sizes": None, "keep": None}
        return c, tuple(range(nE))
    raise KeyError(name)


TABLE_CASES = ["ba", "w1", "w8", "hub"]
DENSE_CASES = ["ba", "w1", "w8"]  # those with identity rows 2 e_i: sigma_min(J) >= 2
DENSE_DAMPING = (0.1, 0.01)

_OPERATORS = {}


def operator(name):
    """(case, eliminate, JacobianOperator, sparse.JacobianSchur) of the named case, built once per process"""
    from baspacho_amd import sparse as S
    if name not in _OPERATORS:
        c, elim = case(name)
        jop = S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
        _OPERATORS[name] = (c, elim, jop, S.JacobianSchur(jop, np.asarray(elim, dtype=np.int64)))
    return _OPERATORS[name]


@functools.lru_cache(maxsize=None)
def model(name, dtype, damped):
    c, elim = case(name)
    return Model(c, elim, dtype, damping_ab=DENSE_DAMPING if damped else None)
