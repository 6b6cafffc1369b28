"""Numpy restatement of the matrix-free least squares of DESIGN.md section 28, for the CPU and GPU tests: the
tables of the JacobianProductMap, the two epilogues, the column norms and the damping vector, the Jacobi and
block-Jacobi builds for J^T J + D, the concatenated fold of the curvature and the whole CGLS iteration with its
state record, in float64 and in float32 with sums in float64.  What the conjugate gradient shares (fold256, dot,
the block factorisation, the applications) is cg_ref's; the products are normal_eq_ref's.  Nothing here touches
the GPU."""
import functools

import numpy as np

import cg_ref as R
import normal_eq_ref as N

LONG_RUN = 64


# ---- the tables ---------------------------------------------------------------------------------------------
def run_list(keys, other, num):
    """(start, entry, index, long_runs): the entries by key, ascending entry index inside a run, with the
    gathered index; the runs of more than 64 entries"""
    keys = np.asarray(keys, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=num))]).astype(np.int32)
    return (start, order.astype(np.int32), np.asarray(other, dtype=np.int64)[order].astype(np.int32),
            np.nonzero(np.diff(start) > LONG_RUN)[0].astype(np.int32))


def block_plan(rows, cols, m, sizes):
    """(block_start, item_start, ka, kb, pos): per block of `sizes` scalars, in ascending Jacobian row, the
    entries x of the row inside the block in ascending entry index, each paired with the entries up to and
    including itself; (ka, kb) ordered so that cols[ka] >= cols[kb], pos = (cols[ka] - s) w + (cols[kb] - s)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    for b, w in enumerate(sizes):
        if w > R.MAX_BLOCK:
            raise ValueError("param %d has %d scalars" % (b, w))
    bs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    blk = np.searchsorted(bs, np.arange(int(bs[-1])), side="right") - 1
    lists = [[] for _ in sizes]
    for ks in N.row_groups(np.asarray(rows, dtype=np.int64), m):
        per = {}
        for k in ks:
            per.setdefault(int(blk[cols[k]]), []).append(int(k))
        for b, es in per.items():
            s, w = int(bs[b]), int(sizes[b])
            for x, a in enumerate(es):
                for e in es[:x + 1]:
                    hi, lo = (a, e) if cols[a] >= cols[e] else (e, a)
                    lists[b].append((hi, lo, (int(cols[hi]) - s) * w + (int(cols[lo]) - s)))
    item_start = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int32)
    flat = [t for b in lists for t in b]
    col = lambda i: np.array([t[i] for t in flat], dtype=np.int32)
    return bs.astype(np.int32), item_start, col(0), col(1), col(2)


# ---- the pieces ---------------------------------------------------------------------------------------------
def epilogue_residual(r, total):
    """res = r + (-sum); r absent: -sum"""
    return (-total) if r is None else (r + (-total)).astype(total.dtype)


def epilogue_normal(total, d, x, c):
    """s = (sum + (-(d x))) + c, the steps of absent operands omitted"""
    dt = total.dtype
    if d is not None:
        total = (total + (-(d[:, None] * x).astype(dt))).astype(dt)
    if c is not None:
        total = (total + c).astype(dt)
    return total


def colsq(cols, n, values, dtype):
    """the squared column norms in float64: the fold in ascending entry index from +0 of double(v) * double(v)"""
    v = np.asarray(values).astype(dtype).astype(np.float64)
    out = np.zeros(n)
    np.add.at(out, np.asarray(cols, dtype=np.int64), v * v)
    return out


def damping(csq, alpha, beta, dtype):
    return (float(alpha) * csq + float(beta)).astype(dtype)


def build_jacobi(csq, d, dtype):
    """(inv [n] dtype, status [2]): inv_i = dtype(1 / (colsq_i + double(d_i))); a denominator that is not
    positive and finite is a bad pivot with inverse 0"""
    den = csq if d is None else csq + d.astype(np.float64)
    ok = (den > 0) & np.isfinite(den)
    with np.errstate(all="ignore"):
        inv = np.where(ok, 1.0 / np.where(ok, den, 1.0), 0.0).astype(dtype)
    bad = np.nonzero(~ok)[0]
    return inv, np.array([bad[0] if len(bad) else -1, len(bad)], dtype=np.int64)


def build_block(plan, values, d, dtype):
    """(minv, block_off, status): G_ab = the block's items added in list order from +0 in float64, each double(v_ka)
    * double(v_kb); double(d) added to the diagonal last; then cg_ref.build_block's factorisation and inverse (run
    in float64 on a plan whose entries are these terms), stored as dtype"""
    bs, start, ka, kb, pos = plan
    v = np.asarray(values).astype(dtype).astype(np.float64)
    terms, tpos, tstart = [], [], [0]
    for b in range(len(bs) - 1):
        s, w = int(bs[b]), int(bs[b + 1] - bs[b])
        sl = slice(start[b], start[b + 1])
        terms.extend(v[ka[sl]] * v[kb[sl]])
        tpos.extend(pos[sl])
        if d is not None:
            terms.extend(d[s:s + w].astype(np.float64))
            tpos.extend(a * w + a for a in range(w))
        tstart.append(len(terms))
    fake = (bs, np.asarray(tstart, dtype=np.int64), np.arange(len(terms)), np.asarray(tpos, dtype=np.int64))
    minv, off, status = R.build_block(fake, np.asarray(terms, dtype=np.float64), np.float64)
    return minv.astype(dtype), off, status


def partials(prod):
    """pass 1 of cg_ref.ordered_sum: [parts, q] partials of the rounded products prod [rows, q]"""
    prod = np.asarray(prod, dtype=np.float64)
    n, q = prod.shape
    parts = (n + R.RED_CHUNK - 1) // R.RED_CHUNK
    pad = np.zeros((parts * R.RED_CHUNK, q))
    pad[:n] = prod
    t = pad.reshape(parts, R.RED_CHUNK // R.RED_THREADS, R.RED_THREADS, q)
    acc = np.zeros((parts, R.RED_THREADS, q))
    for m in range(R.RED_CHUNK // R.RED_THREADS):
        acc = acc + t[:, m]
    return R.fold256(np.moveaxis(acc, 1, 0)) if parts else np.zeros((0, q))


def fold_parts(part):
    """pass 2 of cg_ref.ordered_sum on a list of partials [parts, q]"""
    parts, q = part.shape
    rounds = (parts + R.RED_THREADS - 1) // R.RED_THREADS
    pad = np.zeros((rounds * R.RED_THREADS, q))
    pad[:parts] = part
    acc = np.zeros((R.RED_THREADS, q))
    for k in range(rounds):
        acc = acc + pad[k * R.RED_THREADS:(k + 1) * R.RED_THREADS]
    return R.fold256(acc)


def delta(t, p, d):
    """|J p|^2 + p^T D p: the partials of t.t over the chunks of m, then those of (p p) d over the chunks of n,
    folded as one list"""
    t64, p64 = t.astype(np.float64), p.astype(np.float64)
    parts = partials(t64 * t64)
    if d is not None:
        parts = np.concatenate([parts, partials((p64 * p64) * d.astype(np.float64)[:, None])])
    return fold_parts(parts)


# ---- the iteration ------------------------------------------------------------------------------------------
def cgls_model(case, dtype, r=None, c=None, damping_ab=None, precond=None, tol=1e-10, max_steps=100, x0=None,
               steps=None, values=None):
    """The iteration as the kernels are specified, on the Jacobian `case` (normal_eq_ref's dict).  r [m, q] or
    None, c [n, q] or None; precond None, "jacobi", "block_jacobi" or a callable s -> z.  Returns (x [n, q],
    record, status): record as cg_ref.cg_model's, status the preconditioner's record or None"""
    dt = np.dtype(dtype).type
    rows, cols, m, n = case["rows"], case["cols"], case["m"], case["n"]
    v = np.asarray(case["values"] if values is None else values).astype(dt)
    r = None if r is None else np.asarray(r).astype(dt).reshape(m, -1)
    c = None if c is None else np.asarray(c).astype(dt).reshape(n, -1)
    q = (r if r is not None else c).shape[1]
    jv = lambda x: N.ref_j_vec(rows, cols, m, v, x, dt)
    jtv = lambda u: N.ref_jt_vec(rows, cols, n, v, u, dt)
    csq = colsq(cols, n, v, dt)
    d = None if damping_ab is None else damping(csq, damping_ab[0], damping_ab[1], dt)
    status, apply_m = None, None
    if precond == "jacobi":
        inv, status = build_jacobi(csq, d, dt)
        apply_m = lambda s: R.apply_jacobi(inv, s)
    elif precond == "block_jacobi":
        sizes = np.ones(n, dtype=np.int64) if case["param_sizes"] is None else case["param_sizes"]
        plan = block_plan(rows, cols, m, sizes)
        minv, off, status = build_block(plan, v, d, dt)
        apply_m = lambda s: R.apply_block(plan, minv, off, s)
    elif precond is not None:
        apply_m = precond
    tol2 = float(tol) * float(tol)
    z64 = lambda: np.zeros(q, dtype=np.float64)
    st = {"iterations": np.zeros(q, dtype=np.int64), "stop": np.zeros(q, dtype=np.int64), "rz": z64(), "pAp": z64(),
          "rr": z64(), "bb": z64(), "alpha": z64(), "beta": z64(), "tol2": tol2, "max_steps": int(max_steps)}
    with np.errstate(all="ignore"):
        b = c.copy() if r is None else epilogue_normal(jtv(r), None, None, c)
        bb = R.dot(b, b)
        st["bb"] = bb.copy()
        st["stop"] = np.where(bb == 0, R.ZERO_RHS, np.where(np.isfinite(bb), R.RUNNING, R.NON_FINITE)).astype(np.int64)
        x = np.zeros((n, q), dtype=dt) if x0 is None else np.asarray(x0).astype(dt).reshape(n, -1).copy()
        x[:, st["stop"] == R.ZERO_RHS] = 0
        run = st["stop"] == R.RUNNING
        if x0 is None:
            res = np.zeros((m, q), dtype=dt) if r is None else r.copy()
            s = b.copy()
        else:
            res = np.where(run[None, :], epilogue_residual(r, jv(x)), np.zeros((m, q), dtype=dt))
            s = np.where(run[None, :], epilogue_normal(jtv(res), d, x, c), b)
        p = np.zeros((n, q), dtype=dt)

        def apply_fold(start):
            nonlocal p
            run = st["stop"] == R.RUNNING
            z = s if apply_m is None else np.asarray(apply_m(s)).astype(dt)
            ss, sz = R.dot(s, s), R.dot(s, z)
            if not start:
                st["iterations"] = st["iterations"] + run
            st["rr"] = np.where(run, ss, st["rr"])
            bad = run & ~np.isfinite(ss)
            conv = run & ~bad & (ss <= tol2 * st["bb"])
            lim = run & ~bad & ~conv & (st["iterations"] >= max_steps)
            go = run & ~bad & ~conv & ~lim
            bad2 = go & ~np.isfinite(sz)
            brk = go & ~bad2 & ~(sz > 0)
            go2 = go & ~bad2 & ~brk
            st["beta"] = np.where(go2, np.where(st["iterations"] > 0, sz / st["rz"], 0.0), st["beta"])
            st["rz"] = np.where(go, sz, st["rz"])
            st["stop"] = np.where(bad | bad2, R.NON_FINITE, np.where(conv, R.CONVERGED, np.where(
                lim, R.STEP_LIMIT, np.where(brk, R.BREAKDOWN, st["stop"]))))
            first = st["iterations"] == 0
            pn = np.where(first[None, :], z, (z + (st["beta"].astype(dt)[None, :] * p).astype(dt)).astype(dt))
            p = np.where(go2[None, :], pn, p).astype(dt)

        apply_fold(True)
        for _ in range(max_steps if steps is None else steps):
            if not (st["stop"] == R.RUNNING).any():
                break
            t = jv(p)
            run = st["stop"] == R.RUNNING
            dl = delta(t, p, d)
            st["pAp"] = np.where(run, dl, st["pAp"])
            bad = run & ~np.isfinite(dl)
            brk = run & ~bad & ~(dl > 0)
            go = run & ~bad & ~brk
            st["alpha"] = np.where(go, st["rz"] / dl, st["alpha"])
            st["stop"] = np.where(bad, R.NON_FINITE, np.where(brk, R.BREAKDOWN, st["stop"]))
            a = st["alpha"].astype(dt)[None, :]
            x = np.where(go[None, :], (x + (a * p).astype(dt)).astype(dt), x)
            res = np.where(go[None, :], (res + (-(a * t).astype(dt))).astype(dt), res)
            s = np.where(go[None, :], epilogue_normal(jtv(res), d, x, c), s)
            apply_fold(False)
    return x, st, status


# ---- the Jacobians --------------------------------------------------------------------------------------------
HUB_SIZES = [1, 3, 9, 32, 2] * 2


@functools.lru_cache(maxsize=None)
def hub():
    """m = 130, n = 94: columns 0 .. 3 have 64, 65, 128 and 129 entries, row 129 has 65 entries, column 93 is
    empty, the param sizes cycle through 1, 3, 9, 32, 2.  Every column but the empty one has an entry of
    magnitude >= 2, the rest are uniform in (-1, 1); the entries are shuffled"""
    rng = np.random.default_rng(28)
    m, n = 130, 94
    pos = set()
    for col, cnt in enumerate((64, 65, 128, 129)):
        pos.update((i, col) for i in range(m - cnt, m))
    pos.update((129, j) for j in rng.permutation(np.arange(4, n - 1))[:61])  # with columns 0 .. 3: 65 entries
    pos.update((int(rng.integers(0, 129)), j) for j in range(4, n - 1))
    pos = np.array(sorted(pos), dtype=np.int64)
    vals = rng.uniform(-1, 1, len(pos))
    for j in range(n - 1):
        k = np.nonzero(pos[:, 1] == j)[0][0]
        vals[k] = 2.0 + abs(vals[k])
    order = rng.permutation(len(pos))
    rows, cols = pos[order, 0].copy(), pos[order, 1].copy()
    assert np.bincount(cols, minlength=n)[[0, 1, 2, 3, n - 1]].tolist() == [64, 65, 128, 129, 0]
    assert np.bincount(rows, minlength=m)[129] == 65
    return {"rows": rows, "cols": cols, "values": vals[order], "m": m, "n": n,
            "param_sizes": np.array(HUB_SIZES, dtype=np.int64), "keep": None}


def bidiagonal(m, n, seed=0):
    """J[i, i] = 2 + u_i and J[i + 1, i] = -1 + u'_i / 2 where they fit (u uniform in (0, 1)): full column rank
    for m >= n; for m < n the columns from m on are empty"""
    rng = np.random.default_rng(1000 * m + n + seed)
    k = min(m, n)
    d = np.arange(k, dtype=np.int64)
    lo = d[d + 1 < m]
    rows, cols = np.concatenate([d, lo + 1]), np.concatenate([d, lo])
    vals = np.concatenate([2.0 + rng.uniform(0, 1, k), -1.0 + rng.uniform(0, 0.5, len(lo))])
    order = rng.permutation(len(rows))
    return {"rows": rows[order], "cols": cols[order], "values": vals[order], "m": m, "n": n, "param_sizes": None,
            "keep": None}


def case(name):
    """a Jacobian by name: "hub", "bidiag_<m>_<n>", or one of normal_eq_ref.build's"""
    if name == "hub":
        return hub()
    if name.startswith("bidiag_"):
        _, m, n = name.split("_")
        return bidiagonal(int(m), int(n))
    return N.build(name)


_OPERATORS = {}


def operator(name):
    """(case, JacobianOperator) of the named Jacobian, built once per process"""
    from baspacho_amd import sparse as S
    if name not in _OPERATORS:
        c = case(name)
        _OPERATORS[name] = (c, S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"]))
    return _OPERATORS[name]


def dense_solution(c, r=None, cvec=None, damping_ab=None, values=None):
    """(x, N): the dense float64 solution of (J^T J + D) x = J^T r + c and the matrix"""
    J = N.dense_j(c["m"], c["n"], c["rows"], c["cols"], c["values"] if values is None else values)
    Nm = J.T @ J
    if damping_ab is not None:
        Nm = Nm + np.diag(damping_ab[0] * (J * J).sum(0) + damping_ab[1])
    rhs = 0.0
    if r is not None:
        rhs = rhs + J.T @ np.asarray(r, dtype=np.float64).reshape(c["m"], -1)
    if cvec is not None:
        rhs = rhs + np.asarray(cvec, dtype=np.float64).reshape(c["n"], -1)
    return np.linalg.solve(Nm, rhs), Nm


# (name, scale of the entries outside the identity rows): Jacobians with identity rows 2 e_i, so that sigma_min(J)
# >= 2, scaled so that kappa(J^T J + D) <= 100 with DENSE_DAMPING (both suites check it from the dense matrix)
DENSE_CASES = [("scalar", 1.0), ("blocks", 0.5), ("blocks_elim", 0.5), ("empty_rows", 1.0)]
DENSE_DAMPING = (0.1, 0.01)


def dense_case(name, scale):
    """(case, values) of a DENSE_CASES entry"""
    c = case(name)
    v = c["values"].copy()
    v[v != 2.0] *= scale
    return c, v
