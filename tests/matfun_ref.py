"""Numpy restatement of f(A) v from the Lanczos basis, for the CPU and GPU tests: the
combine kernel (the chain rounded in the value type, the limits, accumulate, several outputs) and the two
drivers of baspacho_amd.lanczos.apply_function on lanczos_ref.lanczos_model: the kept basis, and the second pass
that regenerates v_j on a ring of two slots.  The k x k host work (function_coefficients) is the package's: it is
host code, shared as lanczos_ref's tests share ritz().  Nothing here touches the GPU."""
import numpy as np

from baspacho_amd import lanczos as L
import lanczos_ref as LR
from cg_ref import dot


def combine(vs, y, limit, dtype, out=None, first=0):
    """out_f[:, c] = (out given ? out_f[:, c] : +0) + sum_i dtype(y[c, f, i]) vs[i][:, c], i ascending, every product
    rounded in dtype before it is added; term i is skipped (vs[i] and y[.., i] not used) when first + i >= limit[c].
    vs [count, n, q] (the slots the call is handed), y [q, nf, >= count] float64, limit [q]: [nf, n, q] of dtype"""
    dtype = np.dtype(dtype).type
    vs, y, limit = np.asarray(vs), np.asarray(y, dtype=np.float64), np.asarray(limit)
    count, n, q = vs.shape
    nf = y.shape[1]
    acc = np.zeros((nf, n, q), dtype=dtype) if out is None else np.array(out, dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(count):
            take = (first + i < limit)[None, :]
            for f in range(nf):
                prod = (y[:, f, i].astype(dtype)[None, :] * vs[i].astype(dtype)).astype(dtype)
                acc[f] = np.where(take, (acc[f] + prod).astype(dtype), acc[f])
    return acc


def coefficients(coef, st, fs):
    """the host work of apply_function on a model run: (y [q, nf, steps], limit [q], nan [q], change [nf, q])"""
    q, _, steps = coef.shape
    y = np.zeros((q, len(fs), steps))
    limit = np.zeros(q, dtype=np.int64)
    nan = np.zeros(q, dtype=bool)
    change = np.full((len(fs), q), np.nan)
    for c in range(q):
        k, stop = int(st["steps"][c]), int(st["stop"][c])
        if stop == LR.ZERO_START:
            continue
        if stop == LR.NON_FINITE or k < 1 or not np.isfinite(coef[c, :, :k]).all():
            nan[c] = True
            continue
        limit[c] = k
        vnorm = float(np.sqrt(st["vv"][c]))
        for j, f in enumerate(fs):
            y[c, j, :k] = L.function_coefficients(coef[c, 0], coef[c, 1], k, f, vnorm, c)
            prev = np.zeros(k)
            if k > 1:
                prev[:k - 1] = L.function_coefficients(coef[c, 0], coef[c, 1], k - 1, f, vnorm, c)
            change[j, c] = np.linalg.norm(y[c, j, :k] - prev) / np.linalg.norm(y[c, j, :k])
    return y, limit, nan, change


def ring_pass(n, apply_a, v0, dtype, steps, breakdown=None):
    """The plain three-term recurrence of lanczos_model again, on a ring of two slots: yields (j, ring, slot)
    with ring[slot] = v_j before step j is taken, for j = 0 .. steps - 1; a stopped column's slots keep what they
    held.  The coefficients it meets are returned by the generator's last item as (None, coef, st)"""
    dtype = np.dtype(dtype).type
    v0 = np.asarray(v0).astype(dtype).reshape(n, -1)
    q = v0.shape[1]
    brk = LR.default_breakdown(dtype) if breakdown is None else float(breakdown)
    thr2 = brk * brk
    coef = np.zeros((q, 2, steps))
    ring = np.zeros((min(2, steps), n, q), dtype=dtype)
    with np.errstate(all="ignore"):
        vv = dot(v0, v0)
        stop = np.where(vv == 0, LR.ZERO_START, np.where(np.isfinite(vv), LR.RUNNING, LR.NON_FINITE)).astype(np.int64)
        done = np.zeros(q, dtype=np.int64)
        alpha, beta = np.zeros(q), np.zeros(q)
        run = stop == LR.RUNNING
        ring[0] = np.where(run[None, :], (v0 * (1.0 / np.sqrt(vv)).astype(dtype)[None, :]).astype(dtype), ring[0])
        for j in range(steps):
            yield j, ring, j % 2
            run = stop == LR.RUNNING
            v = ring[j % 2]
            w = np.asarray(apply_a(v)).astype(dtype)
            alpha = np.where(run, dot(v, w), alpha)
            w = (w + (-(alpha.astype(dtype)[None, :] * v).astype(dtype))).astype(dtype)
            if j > 0:
                w = (w + (-(beta.astype(dtype)[None, :] * ring[(j - 1) % 2]).astype(dtype))).astype(dtype)
            ww = dot(w, w)
            beta_prev, b = beta, np.sqrt(ww)
            coef[run, 0, j] = alpha[run]
            coef[run, 1, j] = b[run]
            beta = np.where(run, b, beta)
            done = done + run
            bad = run & ~(np.isfinite(alpha) & np.isfinite(ww))
            inv = run & ~bad & (ww <= thr2 * (alpha * alpha + beta_prev * beta_prev))
            lim = run & ~bad & ~inv & (done >= steps)
            stop = np.where(bad, LR.NON_FINITE, np.where(inv, LR.INVARIANT, np.where(lim, LR.STEP_LIMIT, stop)))
            go = stop == LR.RUNNING
            if j + 1 < steps:
                nxt = (j + 1) % 2
                ring[nxt] = np.where(go[None, :], (w * (1.0 / beta).astype(dtype)[None, :]).astype(dtype), ring[nxt])
    yield None, coef, {"steps": done, "stop": stop}


def apply_function_model(n, apply_a, v0, dtype, fs, steps, reorth="full", memory="basis", breakdown=None):
    """apply_function as specified: (out [nf, n, q] dtype, info) with info = dict of steps, stop, change, limit"""
    dtype = np.dtype(dtype).type
    if memory == "two_pass" and reorth is not None:
        raise ValueError("two_pass needs reorth=None")
    coef, st, V = LR.lanczos_model(n, apply_a, v0, dtype, steps, reorth, breakdown)
    y, limit, nan, change = coefficients(coef, st, fs)
    q = coef.shape[0]
    if memory == "basis":
        out = combine(V, y, limit, dtype)
    else:
        out = None
        last = max(int(limit.max(initial=0)), 1)
        for j, ring, slot in ring_pass(n, apply_a, v0, dtype, steps, breakdown):
            if j is None or j >= last:
                break   # the device queues no step behind v_{last - 1}
            out = combine(ring[slot:slot + 1], y[:, :, j:j + 1], limit, dtype, out=out, first=j)
    out[:, :, nan] = np.nan
    return out, {"steps": st["steps"], "stop": st["stop"], "change": change, "limit": limit, "coef": coef}


def dense_function(A, f, v):
    """U f(Lambda) U^T v in float64 from numpy.linalg.eigh"""
    lam, U = np.linalg.eigh(np.asarray(A, dtype=np.float64))
    return U @ (L._function_values(f, lam, "", {})[:, None] * (U.T @ np.asarray(v, dtype=np.float64).reshape(len(lam), -1)))


def rel_err(got, want):
    """relative 2-norm error per column"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.linalg.norm(got - want, axis=0) / np.linalg.norm(want, axis=0)
