"""numpy restatement of the factor status and of the damping of the diagonal (DESIGN.md section 18;
csrc/hip_status_kernels.h), and the dense column Cholesky that says where a factor must break.

  scan(sol, host_data, spanBegin, spanEnd)   the four words of bsp_factor_status_* from diagOffsets()
  damp(sol, host_data, alpha, beta, ...)     bsp_damp_* with scalars of the data's dtype, on a copy
  nan_cholesky(dense_lower)                  column Cholesky in the given order that lets NaN propagate
  first_failing_pivot(dense_lower)           the first column whose pivot is not finite and positive

Nothing here touches the GPU."""
import numpy as np

INF_BITS = int(np.array([np.inf]).view(np.int64)[0])


def scalar_range(sol, spanBegin=0, spanEnd=None):
    ss = sol.skel()["spanStart"]
    spanEnd = sol.numSpans() if spanEnd is None else spanEnd
    assert 0 <= spanBegin <= spanEnd <= sol.numSpans()
    return int(ss[spanBegin]), int(ss[spanEnd])


def is_good(d):
    """positive and finite in the array's own dtype"""
    d = np.asarray(d)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def scan(sol, host_data, spanBegin=0, spanEnd=None):
    """int64 [4]: {lowest bad internal scalar or -1, bad diagonals, bits of the float64 minimum over the
    good diagonals (+inf: none), bits of the float64 maximum (0.0: none)}"""
    host_data = np.asarray(host_data)
    g0, g1 = scalar_range(sol, spanBegin, spanEnd)
    d = host_data[sol.diagOffsets()[g0:g1]]
    good = is_good(d)
    bad = np.nonzero(~good)[0]
    wide = d[good].astype(np.float64)  # exact for float32
    mn = wide.min() if wide.size else np.inf
    mx = wide.max() if wide.size else 0.0
    bits = np.array([mn, mx], dtype=np.float64).view(np.int64)
    return np.array([g0 + int(bad[0]) if bad.size else -1, bad.size, bits[0], bits[1]], dtype=np.int64)


def damp(sol, host_data, alpha, beta, spanBegin=0, spanEnd=None):
    """a copy of host_data with d <- (d * (1 + alpha)) + beta on the diagonals of the range, every
    operation on scalars of the data's dtype (three roundings)"""
    out = np.array(host_data, copy=True)
    T = out.dtype.type
    g0, g1 = scalar_range(sol, spanBegin, spanEnd)
    idx = sol.diagOffsets()[g0:g1]
    t = T(1) + T(alpha)
    out[idx] = out[idx] * t + T(beta)
    assert out.dtype == np.asarray(host_data).dtype
    return out


def nan_cholesky(dense_lower):
    """left-looking column Cholesky of the symmetric matrix given by its lower triangle, float64, in the
    given (internal) order.  No pivot is tested: the square root of a negative pivot is NaN and
    propagates to everything computed from it -- and to nothing else"""
    A = np.tril(np.asarray(dense_lower, dtype=np.float64))
    n = A.shape[0]
    L = np.zeros_like(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(n):
            v = A[j:, j] - L[j:, :j] @ L[j, :j]
            L[j:, j] = v / np.sqrt(v[0])
            L[j, j] = np.sqrt(v[0])
    return L


def first_failing_pivot(dense_lower):
    """the first column j whose pivot A_jj - sum_k L_jk^2 is not finite and positive (-1: none), the
    columns before it factored exactly as nan_cholesky does"""
    A = np.tril(np.asarray(dense_lower, dtype=np.float64))
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not (np.isfinite(v[0]) and v[0] > 0):
            return j
        L[j:, j] = v / np.sqrt(v[0])
    return -1


def plant_negative(sol, host_data, k):
    """a copy of host_data with A_kk <- -|A_kk| - 1 at internal scalar k"""
    out = np.array(host_data, copy=True)
    at = int(sol.diagOffsets()[k])
    out[at] = -abs(out[at]) - out.dtype.type(1)
    return out


def decode(words):
    """(first, count, minDiag, maxDiag) of a record"""
    w = np.asarray(words, dtype=np.int64).reshape(4)
    mn, mx = w[2:4].copy().view(np.float64)
    return int(w[0]), int(w[1]), float(mn), float(mx)
