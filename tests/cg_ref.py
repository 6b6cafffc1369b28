"""Numpy restatement of the device-resident conjugate gradient of DESIGN.md section 24, for the CPU and GPU
tests: the two-pass ordered sum of the dot products, the product A p in the order of sym_product_ref (a
vectorised form of its fold, checked against it by the CPU tests), the plans, builds and applications of the
Jacobi and block-Jacobi preconditioners, and the whole iteration with its state record, masking and stop
reasons, in float64 and in float32 with sums in float64.  Nothing here touches the GPU.

error_bounds_ref.py states maxRatio and colMax, whose merges do not depend on the order, so it has no fold of
sums to import; the fold of the reduction convention is stated here (fold256)."""
import functools
import math

import numpy as np

from sym_product_ref import kept_entries, row_terms

RED_THREADS, RED_CHUNK = 256, 1024
STOPS = ("running", "converged", "step limit", "breakdown", "non-finite", "zero right-hand side")
RUNNING, CONVERGED, STEP_LIMIT, BREAKDOWN, NON_FINITE, ZERO_RHS = range(6)
MAX_BLOCK = 32


def fold256(v):
    """the LDS fold of 256 thread values (axis 0): for s = 128 .. 1, entry t < s becomes entry t + entry t + s"""
    v = np.array(v, dtype=np.float64)
    s = RED_THREADS // 2
    while s:
        v[:s] = v[:s] + v[s:2 * s]
        s //= 2
    return v[0]


def ordered_sum(prod):
    """per column of prod [n, q] (float64, the rounded products): pass 1, chunk x owns the rows [1024 x, 1024
    (x + 1)), thread t adds the rows 1024 x + 256 m + t, m = 0 .. 3, from +0, fold256; pass 2, thread t adds the
    partials t, t + 256, ... from +0, fold256.  (A missing row adds nothing; here it adds +0.0, which cannot
    change a sum that started from +0.0.)"""
    prod = np.asarray(prod, dtype=np.float64)
    n, q = prod.shape
    parts = (n + RED_CHUNK - 1) // RED_CHUNK
    if parts == 0:
        return np.zeros(q)
    pad = np.zeros((parts * RED_CHUNK, q))
    pad[:n] = prod
    t = pad.reshape(parts, RED_CHUNK // RED_THREADS, RED_THREADS, q)
    acc = np.zeros((parts, RED_THREADS, q))
    for m in range(RED_CHUNK // RED_THREADS):
        acc = acc + t[:, m]
    part = fold256(np.moveaxis(acc, 1, 0))  # [parts, q]
    rounds = (parts + RED_THREADS - 1) // RED_THREADS
    pad2 = np.zeros((rounds * RED_THREADS, q))
    pad2[:parts] = part
    acc2 = np.zeros((RED_THREADS, q))
    for k in range(rounds):
        acc2 = acc2 + pad2[k * RED_THREADS:(k + 1) * RED_THREADS]
    return fold256(acc2)


def dot(a, b):
    """a.b per column of [n, q] arrays: operands to float64, every product rounded, ordered_sum"""
    return ordered_sum(a.astype(np.float64) * b.astype(np.float64))


def run_fold(start, terms, dtype):
    """per run u the terms [start[u], start[u + 1]) (terms [T, q]) added one by one from +0 in `dtype`"""
    lens = np.diff(start)
    out = np.zeros((len(lens),) + terms.shape[1:], dtype=dtype)
    for t in range(int(lens.max()) if len(lens) else 0):
        u = np.nonzero(lens > t)[0]
        out[u] = (out[u] + terms[start[u] + t]).astype(dtype)
    return out


class Product:
    """y = A x from the entries in the order of sym_product_ref.mv_model, vectorised over the rows"""

    def __init__(self, n, rows, cols, triangle="lower"):
        self.n, self.triangle = n, triangle
        self.rows, self.cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        self.start, self.entry, self.index, _ = row_terms(n, self.rows, self.cols, triangle)
        self.start = self.start.astype(np.int64)

    def mv(self, values, x, dtype):
        v = np.asarray(values).astype(dtype)
        x2 = np.asarray(x).astype(dtype).reshape(self.n, -1)
        terms = (v[self.entry][:, None] * x2[self.index]).astype(dtype)
        return run_fold(self.start, terms, dtype).reshape(np.shape(x))


# ---- the built-in preconditioners ------------------------------------------------------------------------
def precond_plan(n, rows, cols, triangle, block_sizes=None):
    """the host plan restated: (block_start [nb + 1], item_start [nb + 1], entry [items], pos [items]).  The
    items of block b, in ascending entry index, are the kept entries (i, j), i >= j, with both scalars in the
    block, at pos = (i - s) w + (j - s).  block_sizes None: every scalar is a block (Jacobi)"""
    sizes = np.ones(n, dtype=np.int64) if block_sizes is None else np.asarray(block_sizes, dtype=np.int64)
    for b, w in enumerate(sizes):
        if w > MAX_BLOCK:
            raise ValueError("param %d has %d scalars" % (b, w))
    bs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert bs[-1] == n
    blk = np.searchsorted(bs, np.arange(n), side="right") - 1
    keep = kept_entries(n, rows, cols, triangle)
    lists = [[] for _ in sizes]
    for k in range(len(rows)):
        i, j = int(rows[k]), int(cols[k])
        if keep[k] and blk[i] == blk[j]:
            s = int(bs[blk[i]])
            lists[blk[i]].append((k, (i - s) * int(sizes[blk[i]]) + (j - s)))
    item_start = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int32)
    flat = [t for b in lists for t in b]
    return (bs.astype(np.int32), item_start, np.array([t[0] for t in flat], dtype=np.int32),
            np.array([t[1] for t in flat], dtype=np.int32))


def _finite_pos(d):
    return d > 0.0 and math.isfinite(d)


def build_jacobi(plan, values, dtype):
    """(inv [n] dtype, status [2]): d_i = the diagonal entries of scalar i added in ascending entry index from
    +0 in float64, inv_i = dtype(1 / d_i); a d that is not positive and finite is a bad pivot with inverse 0"""
    bs, start, entry, _ = plan
    v = np.asarray(values).astype(dtype).astype(np.float64)
    d = run_fold(start.astype(np.int64), v[entry], np.float64)
    ok = (d > 0) & np.isfinite(d)
    with np.errstate(all="ignore"):
        inv = np.where(ok, (1.0 / np.where(ok, d, 1.0)), 0.0).astype(dtype)
    bad = np.nonzero(~ok)[0]
    return inv, np.array([bs[bad[0]] if len(bad) else -1, len(bad)], dtype=np.int64)


def build_block(plan, values, dtype):
    """(minv, block_off, status): per block, in float64 scalars with every product rounded before it is added:
    the entries summed in ascending entry index, Cholesky column by column, L^-1 by forward substitution, the
    inverse M^-1_ij = sum_{k >= max(i, j)} L^-1_ki L^-1_kj (k ascending), stored as dtype, row-major.  The
    inverse of a block with a bad pivot is zero; status = {block start + pivot of the lowest bad block or -1,
    number of bad blocks}"""
    bs, start, entry, pos = plan
    v = np.asarray(values).astype(dtype)
    nb = len(bs) - 1
    widths = np.diff(bs).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(widths * widths)])
    minv = np.zeros(int(off[-1]), dtype=dtype)
    first, count = -1, 0
    for b in range(nb):
        w = int(widths[b])
        A = [0.0] * (w * w)
        for t in range(start[b], start[b + 1]):
            A[pos[t]] = A[pos[t]] + float(v[entry[t]])
        bad = -1
        for k in range(w):
            d = A[k * w + k]
            if not _finite_pos(d):
                bad = k
                break
            s = math.sqrt(d)
            A[k * w + k] = s
            for i in range(k + 1, w):
                A[i * w + k] = A[i * w + k] / s
            for i in range(k + 1, w):
                for c in range(k + 1, i + 1):
                    A[i * w + c] = A[i * w + c] + (-(A[i * w + k] * A[c * w + k]))
        if bad >= 0:
            count += 1
            if first < 0:
                first = int(bs[b]) + bad
            continue
        Li = [0.0] * (w * w)
        for c in range(w):
            Li[c * w + c] = 1.0 / A[c * w + c]
            for i in range(c + 1, w):
                s = 0.0
                for k in range(c, i):
                    s = s + A[i * w + k] * Li[k * w + c]
                Li[i * w + c] = -s / A[i * w + i]
        out = np.zeros(w * w)
        for i in range(w):
            for c in range(w):
                s = 0.0
                for k in range(max(i, c), w):
                    s = s + Li[k * w + i] * Li[k * w + c]
                out[i * w + c] = s
        minv[off[b]:off[b + 1]] = out.astype(dtype)
    return minv, off, np.array([first, count], dtype=np.int64)


def apply_jacobi(inv, r):
    return (r * inv[:, None]).astype(r.dtype)


def apply_block(plan, minv, off, r):
    """z_i = dtype(sum_j float64(Minv_ij) float64(r_j)) over the block of i, j ascending"""
    bs = plan[0]
    z = np.zeros_like(r)
    for b in range(len(bs) - 1):
        s0, w = int(bs[b]), int(bs[b + 1] - bs[b])
        M = minv[off[b]:off[b + 1]].reshape(w, w).astype(np.float64)
        R = r[s0:s0 + w].astype(np.float64)
        s = np.zeros((w, r.shape[1]))
        for j in range(w):
            s = s + M[:, j:j + 1] * R[j][None, :]
        z[s0:s0 + w] = s.astype(r.dtype)
    return z


# ---- the iteration ------------------------------------------------------------------------------------------
def cg_model(n, apply_a, b, dtype, apply_m=None, tol=1e-10, max_steps=100, x0=None, steps=None):
    """The iteration as the kernels are specified.  apply_a(p) -> A p and apply_m(r) -> z on [n, q] arrays of
    `dtype` (apply_m None: plain CG).  Returns (x [n, q], record): record = dict of [q] arrays iterations,
    stop (int64) and rz, pAp, rr, bb, alpha, beta (float64), tol2, max_steps.  steps: how many iterations to
    take (default max_steps): stopped columns are frozen, so more steps never change them"""
    dtype = np.dtype(dtype).type
    b = np.asarray(b).astype(dtype).reshape(n, -1)
    q = b.shape[1]
    plain = apply_m is None
    tol2 = float(tol) * float(tol)
    z64 = lambda: np.zeros(q, dtype=np.float64)
    st = {"iterations": np.zeros(q, dtype=np.int64), "stop": np.zeros(q, dtype=np.int64), "rz": z64(), "pAp": z64(),
          "rr": z64(), "bb": z64(), "alpha": z64(), "beta": z64(), "tol2": tol2, "max_steps": int(max_steps)}
    with np.errstate(all="ignore"):
        if x0 is None:
            x, r = np.zeros_like(b), b.copy()
        else:
            x = np.asarray(x0).astype(dtype).reshape(n, -1).copy()
            r = (b + (-apply_a(x))).astype(dtype)
        p = np.zeros_like(b)
        bb = dot(b, b)
        st["bb"] = bb.copy()
        st["stop"] = np.where(bb == 0, ZERO_RHS, np.where(np.isfinite(bb), RUNNING, NON_FINITE)).astype(np.int64)
        zero = st["stop"] == ZERO_RHS
        x[:, zero] = 0
        r[:, zero] = 0

        def rr_fold(count):
            run = st["stop"] == RUNNING
            rr = dot(r, r)
            st["rr"] = np.where(run, rr, st["rr"])
            if count:
                st["iterations"] = st["iterations"] + run
            bad = run & ~np.isfinite(rr)
            conv = run & ~bad & (rr <= tol2 * st["bb"])
            lim = run & ~bad & ~conv & (st["iterations"] >= max_steps)
            st["stop"] = np.where(bad, NON_FINITE, np.where(conv, CONVERGED, np.where(lim, STEP_LIMIT, st["stop"])))
            go = run & ~bad & ~conv & ~lim
            if plain:
                st["beta"] = np.where(go, rr / st["rz"] if count else 0.0, st["beta"])
                st["rz"] = np.where(go, rr, st["rz"])

        def direction():
            nonlocal p
            run = st["stop"] == RUNNING
            if plain:
                z = r
            else:
                z = np.asarray(apply_m(r)).astype(dtype)
                rz = dot(r, z)
                bad = run & ~np.isfinite(rz)
                brk = run & ~bad & ~(rz > 0)
                go = run & ~bad & ~brk
                st["beta"] = np.where(go, np.where(st["iterations"] > 0, rz / st["rz"], 0.0), st["beta"])
                st["rz"] = np.where(run, rz, st["rz"])
                st["stop"] = np.where(bad, NON_FINITE, np.where(brk, BREAKDOWN, st["stop"]))
                run = go
            first = st["iterations"] == 0
            pn = np.where(first[None, :], z, (z + (st["beta"].astype(dtype)[None, :] * p).astype(dtype)).astype(dtype))
            p = np.where(run[None, :], pn, p).astype(dtype)

        rr_fold(False)
        direction()
        for _ in range(max_steps if steps is None else steps):
            if not (st["stop"] == RUNNING).any():
                break
            ap = np.asarray(apply_a(p)).astype(dtype)
            run = st["stop"] == RUNNING
            pap = dot(p, ap)
            st["pAp"] = np.where(run, pap, st["pAp"])
            bad = run & ~np.isfinite(pap)
            brk = run & ~bad & ~(pap > 0)
            go = run & ~bad & ~brk
            st["alpha"] = np.where(go, st["rz"] / pap, st["alpha"])
            st["stop"] = np.where(bad, NON_FINITE, np.where(brk, BREAKDOWN, st["stop"]))
            a = st["alpha"].astype(dtype)[None, :]
            x = np.where(go[None, :], (x + (a * p).astype(dtype)).astype(dtype), x)
            r = np.where(go[None, :], (r + (-(a * ap).astype(dtype))).astype(dtype), r)
            rr_fold(True)
            direction()
    return x, st


def entries_model(n, rows, cols, values, b, dtype, precond=None, param_sizes=None, triangle="lower", **kw):
    """cg_model on a matrix given by entries with a built-in preconditioner (None, "jacobi", "block_jacobi"):
    (x, record, status) with status the preconditioner's record or None"""
    prod = Product(n, rows, cols, triangle)
    dt = np.dtype(dtype).type
    status, apply_m = None, None
    if precond == "jacobi":
        plan = precond_plan(n, rows, cols, triangle)
        inv, status = build_jacobi(plan, values, dt)
        apply_m = lambda r: apply_jacobi(inv, r)
    elif precond == "block_jacobi":
        plan = precond_plan(n, rows, cols, triangle, np.ones(n, dtype=np.int64) if param_sizes is None else param_sizes)
        minv, off, status = build_block(plan, values, dt)
        apply_m = lambda r: apply_block(plan, minv, off, r)
    elif precond is not None:
        apply_m = precond
    x, st = cg_model(n, lambda p: prod.mv(values, p, dt), b, dt, apply_m, **kw)
    return x.reshape(np.shape(b)), st, status


def record_words(st, j):
    """the 12 words of column j of a record, as the device holds them"""
    f = np.array([st[k][j] for k in ("rz", "pAp", "rr", "bb", "alpha", "beta")] + [st["tol2"]], dtype=np.float64)
    return np.concatenate([[st["iterations"][j], st["stop"][j]], f.view(np.int64), [st["max_steps"], 0, 0]]).astype(np.int64)


# ---- the matrices ------------------------------------------------------------------------------------------
def tridiagonal(n, diag=2.5, off=-1.0):
    """lower entries of the tridiagonal Toeplitz matrix (diag, off): eigenvalues in [diag - 2 |off|, diag + 2 |off|]"""
    d = np.arange(n, dtype=np.int64)
    rows, cols = np.concatenate([d, d[1:]]), np.concatenate([d, d[:-1]])
    return rows, cols, np.concatenate([np.full(n, diag), np.full(n - 1, off)])


def block_sparse(sizes, seed, c=None, kappa=1e3):
    """(rows, cols, values, A): the lower entries (block by block, shuffled) of A = G G^T + c I with G block
    sparse over params of `sizes`, c chosen so that kappa_2(A) = kappa (A's own c when given)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)
    n, nb = int(sizes.sum()), len(sizes)
    bs = np.concatenate([[0], np.cumsum(sizes)])
    G = np.zeros((n, n))
    for b in range(nb):
        for o in {b, (b + 1) % nb, int(rng.integers(nb))}:
            G[bs[b]:bs[b + 1], bs[o]:bs[o + 1]] = rng.uniform(-1, 1, (sizes[b], sizes[o]))
    M = G @ G.T
    M = (M + M.T) / 2
    ev = np.linalg.eigvalsh(M)
    if c is None:
        c = max((ev[-1] - kappa * ev[0]) / (kappa - 1), 1e-3 * ev[-1])
    A = M + c * np.eye(n)
    i, j = np.nonzero(np.tril(A))
    order = rng.permutation(len(i))
    i, j = i[order].astype(np.int64), j[order].astype(np.int64)
    return i, j, A[i, j].copy(), A


# the block-sparse matrix both suites use: G G^T + c I over params of mixed sizes, kappa_2 = 1e3
BS_SIZES = [3, 1, 9, 2, 3, 1, 9, 4, 3, 5]
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def bs_case():
    """(rows, cols, values, A, n)"""
    rows, cols, values, A = block_sparse(BS_SIZES, seed=5)
    return rows, cols, values, A, int(np.sum(BS_SIZES))


def cg_bound(kappa, tol):
    """the textbook step bound: |e_k|_A <= 2 ((sqrt k - 1) / (sqrt k + 1))^k |e_0|_A, and |r| / |b| <= sqrt(kappa)
    |e_k|_A / |e_0|_A for x0 = 0, so the steps to tol are at most log(tol / (2 sqrt kappa)) / log(rho), rounded up"""
    rho = (math.sqrt(kappa) - 1) / (math.sqrt(kappa) + 1)
    return int(math.ceil(math.log(tol / (2 * math.sqrt(kappa))) / math.log(rho)))
