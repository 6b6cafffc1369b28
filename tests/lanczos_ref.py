"""Numpy restatement of the device-resident Lanczos recurrence of DESIGN.md section 25, for the CPU and GPU
tests: the recurrence with its state record, coefficients, basis, masking and stop reasons, in float64 and in
float32 with sums in float64.  The two-pass ordered sum, the product A v and the test matrices are cg_ref's.
Nothing here touches the GPU."""
import numpy as np

from cg_ref import Product, dot, fold256, ordered_sum, tridiagonal  # noqa: F401  (fold256 and tridiagonal for the tests)

STOPS = ("running", "unused", "step limit", "invariant subspace", "non-finite", "zero start vector")
RUNNING, STEP_LIMIT, INVARIANT, NON_FINITE, ZERO_START = 0, 2, 3, 4, 5


def default_breakdown(dtype):
    return 64.0 * float(np.finfo(np.dtype(dtype)).eps)


def subtract(w, c, vs, dtype):
    """w - dtype(c_i) v_i for i ascending, every product rounded before it is subtracted.  w [n, q], c [k, q]
    (float64), vs [k, n, q]"""
    w = np.asarray(w, dtype=dtype)
    for i in range(len(vs)):
        w = (w + (-(np.asarray(c[i]).astype(dtype)[None, :] * vs[i]).astype(dtype))).astype(dtype)
    return w


def project(vs, w):
    """c_i = v_i . w per column, i over vs [k, n, q]: [k, q] float64.  Every sum is dot()'s; the k sums are taken
    in one call, which does not change their bits"""
    k, n, q = vs.shape
    prod = vs.astype(np.float64) * w.astype(np.float64)[None]
    return ordered_sum(np.moveaxis(prod, 0, 1).reshape(n, k * q)).reshape(k, q)


def lanczos_model(n, apply_a, v0, dtype, steps, reorth="full", breakdown=None):
    """The recurrence as the kernels are specified.  apply_a(v) -> A v on [n, q] arrays of `dtype`.  Returns
    (coef [q, 2, steps] float64, record, V [steps, n, q] dtype): record = dict of [q] arrays steps, stop (int64)
    and vv, alpha, beta, ww (float64), thr2, kmax; V[j] = v_j, zero where a column never wrote it"""
    dtype = np.dtype(dtype).type
    v0 = np.asarray(v0).astype(dtype).reshape(n, -1)
    q = v0.shape[1]
    brk = default_breakdown(dtype) if breakdown is None else float(breakdown)
    thr2 = brk * brk
    z64 = lambda: np.zeros(q, dtype=np.float64)
    st = {"steps": np.zeros(q, dtype=np.int64), "stop": np.zeros(q, dtype=np.int64), "vv": z64(), "alpha": z64(),
          "beta": z64(), "ww": z64(), "thr2": thr2, "kmax": int(steps)}
    coef = np.zeros((q, 2, steps), dtype=np.float64)
    V = np.zeros((steps, n, q), dtype=dtype)
    with np.errstate(all="ignore"):
        vv = dot(v0, v0)
        st["vv"] = vv.copy()
        st["stop"] = np.where(vv == 0, ZERO_START, np.where(np.isfinite(vv), RUNNING, NON_FINITE)).astype(np.int64)
        run = st["stop"] == RUNNING
        scale = (1.0 / np.sqrt(vv)).astype(dtype)
        V[0] = np.where(run[None, :], (v0 * scale[None, :]).astype(dtype), V[0])
        for j in range(steps):
            run = st["stop"] == RUNNING
            if not run.any():
                break
            w = np.asarray(apply_a(V[j])).astype(dtype)
            st["alpha"] = np.where(run, dot(V[j], w), st["alpha"])
            w = (w + (-(st["alpha"].astype(dtype)[None, :] * V[j]).astype(dtype))).astype(dtype)
            if j > 0:
                w = (w + (-(st["beta"].astype(dtype)[None, :] * V[j - 1]).astype(dtype))).astype(dtype)
            if reorth == "full":
                for _ in range(2):
                    c = project(V[:j + 1], w)
                    w = subtract(w, c, V[:j + 1], dtype)
            ww = dot(w, w)
            beta_prev = st["beta"]
            beta = np.sqrt(ww)
            coef[run, 0, j] = st["alpha"][run]
            coef[run, 1, j] = beta[run]
            st["beta"] = np.where(run, beta, st["beta"])
            st["ww"] = np.where(run, ww, st["ww"])
            st["steps"] = st["steps"] + run
            a = st["alpha"]
            bad = run & ~(np.isfinite(a) & np.isfinite(ww))
            inv = run & ~bad & (ww <= thr2 * (a * a + beta_prev * beta_prev))
            lim = run & ~bad & ~inv & (st["steps"] >= steps)
            st["stop"] = np.where(bad, NON_FINITE, np.where(inv, INVARIANT, np.where(lim, STEP_LIMIT, st["stop"])))
            go = st["stop"] == RUNNING
            if j + 1 < steps:
                V[j + 1] = np.where(go[None, :], (w * (1.0 / st["beta"]).astype(dtype)[None, :]).astype(dtype), V[j + 1])
    return coef, st, V


def entries_model(n, rows, cols, values, v0, dtype, steps, triangle="lower", **kw):
    """lanczos_model on a matrix given by entries"""
    prod = Product(n, rows, cols, triangle)
    dt = np.dtype(dtype).type
    return lanczos_model(n, lambda v: prod.mv(values, v, dt), v0, dt, steps, **kw)


def record_words(st, c):
    """the 12 words of column c of a record, as the device holds them"""
    f = np.array([st[k][c] for k in ("vv", "alpha", "beta", "ww")] + [st["thr2"]], dtype=np.float64)
    return np.concatenate([[st["steps"][c], st["stop"][c]], f.view(np.int64), [st["kmax"], 0, 0, 0, 0]]).astype(np.int64)
