"""Matrices with a known factor, and checks scaled to the working precision.

`spd_data` (helpers.py) raises the diagonal by about the order of the matrix: the Schur updates are
then 1e-4 .. 1e-6 of the factor, and a kernel that drops a tile update or rounds an f64 update through
f32 still lands within the parity tests' fixed tolerances.  Here A = L0 L0^T for a random L0 on the
solver's stored pattern with off-diagonals of the size of the diagonal, so every update matters, and
the tolerances are C * u(dtype) with one constant C per metric and dtype (the unit roundoff u).

The reference is always the float64 Cholesky factor (and float64 solve) of the data as it is passed
to the device, after rounding to the working precision; L0 is only the generator.

tests/test_known_factor_cpu.py simulates correct and deliberately wrong blocked factors and solves in
numpy and asserts that the checks pass the former and fail the latter, each by at least 10x.

Partial factors (factorUpTo(k) at the column bar = spanStart[k]) are checked on the leading columns
(lead_off, lead_diag, lead_backward) and on the Schur complement S = A22 - L21 L21^T left in the
trailing block (schur); trailing entries that no cross-cut product reaches must keep their input
bitwise.  tests/test_partial_factor_cpu.py proves those checks in numpy the same way.
"""
import atexit
import json
import os

import numpy as np

UNIT_ROUNDOFF = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}

# C of every metric, tolerance = C * u(dtype).  The device's errors on correct paths stay within
# about C / 10 (measured over test_known_factor_gpu.py and the stress slice: at most 5 u for the factor
# metrics, 12 u forward and 3 u backward for the solves, both precisions), and the simulated mistakes
# of test_known_factor_cpu.py exceed 10 C.  The partial-factor metrics (lead_*, schur) were fixed
# before their first device run at the values of the factor metrics they restrict; their simulated
# mistakes (test_partial_factor_cpu.py) exceed 10 C as well.
_PARTIAL_C = {"lead_off": 128.0, "lead_diag": 128.0, "lead_backward": 64.0, "schur": 128.0}
C = {
    np.dtype(np.float64): {"off": 128.0, "diag": 128.0, "backward": 64.0,
                           "solve_forward": 512.0, "solve_backward": 64.0, **_PARTIAL_C},
    np.dtype(np.float32): {"off": 128.0, "diag": 128.0, "backward": 64.0,
                           "solve_forward": 512.0, "solve_backward": 64.0, **_PARTIAL_C},
}


def tolerance(metric, dtype):
    dt = np.dtype(dtype)
    return C[dt][metric] * UNIT_ROUNDOFF[dt]


def sparsify(sol, dense, dtype=np.float64):
    """inverse of Solver.densify: the numeric layout of the lower triangle of `dense` on the solver's
    stored pattern (the strictly-upper entries of the square diagonal blocks, which the factor never
    reads, hold the upper triangle's values)"""
    sk = sol.skel()
    out = np.zeros(sol.dataSize(), dtype=dtype)
    ls, ss = sk["lumpStart"], sk["spanStart"]
    for l in range(sol.numLumps()):
        c0, w = int(ls[l]), int(ls[l + 1] - ls[l])
        for c in range(int(sk["chainColPtr"][l]), int(sk["chainColPtr"][l + 1])):
            sp = int(sk["chainRowSpan"][c])
            r0, rows = int(ss[sp]), int(ss[sp + 1] - ss[sp])
            d0 = int(sk["chainData"][c])
            out[d0:d0 + rows * w] = dense[r0:r0 + rows, c0:c0 + w].ravel()
    return out


def stored_pattern(sol):
    """dense boolean lower triangle of the stored pattern (diagonal included)"""
    ones = np.ones(sol.dataSize())
    return np.tril(sol.densify(ones)) != 0


def data_index(sol):
    """dense int64 matrix: the position in the numeric data of each stored lower entry, -1 elsewhere"""
    pos = np.arange(1, sol.dataSize() + 1, dtype=np.float64)
    return np.tril(sol.densify(pos)).astype(np.int64) - 1


def leading_words(sol, span):
    """the numeric data of the lump columns before `span` (a lump boundary) is one leading stretch
    data[:end]; returns end (asserted against the layout)"""
    sk = sol.skel()
    lump = int(sk["spanToLump"][span])
    end = int(sk["chainData"][sk["chainColPtr"][lump]]) if lump < sol.numLumps() else sol.dataSize()
    bar = int(sk["spanStart"][span])
    idx = data_index(sol)
    assert np.all(idx[:, :bar][idx[:, :bar] >= 0] < end) and np.all(idx[:, bar:][idx[:, bar:] >= 0] >= end)
    return end


def bitwise_equal(a, b):
    """equal words (NaN payloads included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return np.array_equal(a.view(u), b.view(u))


class KnownFactor:
    """one matrix: `data` (host, in `dtype`, the solver's layout), its float64 dense form `A` and the
    float64 reference factor `L` of exactly that data"""

    def __init__(self, sol, data, A, L, pattern):
        self.sol, self.data, self.A, self.L, self.pattern = sol, data, A, L, pattern
        self.dtype = data.dtype

    def factor_errors(self, got):
        """relative errors of the strictly-lower entries and of the diagonal (on the stored pattern,
        separately: together, the diagonal dominates the norm) and the backward error
        ||A - G G^T||_F / ||A||_F of a factor G in the solver's layout"""
        G = np.tril(self.sol.densify(np.asarray(got, dtype=np.float64)))
        G[~self.pattern] = 0.0
        return factor_errors_dense(G, self.L, self.A, self.pattern)

    def solve_errors(self, b, x, op="A"):
        return solve_errors(self.operator(op), b, x)

    def operator(self, op):
        return {"A": self.A, "L": self.L, "Lt": self.L.T}[op]

    def check_factor(self, got, what=""):
        check(self.factor_errors(got), self.dtype, what)

    def check_solve(self, b, x, op="A", what=""):
        check(self.solve_errors(b, x, op), self.dtype, what)

    # ---- partial factors: factorUpTo(k), bar = spanStart[k]
    def partial_errors_dense(self, G, bar):
        """lead_off / lead_diag: relative errors of the stored entries of columns < bar (strictly lower,
        diagonal); lead_backward: ||A[:, :bar] - G[:, :bar] G[:bar, :bar]^T|| / ||A[:, :bar]||; schur:
        ||S_dev - S_ref|| / (||A22|| + ||L21 L21^T||) on the lower stored pattern of the trailing block,
        S_ref = A22 - L21 L21^T (G: dense, lower, float64)"""
        P, L, A = self.pattern, self.L, self.A
        G = np.where(P, G, 0.0)
        strict = np.tril(P, -1)
        strict[:, bar:] = False
        ref_off = np.linalg.norm(L[strict])
        off = np.linalg.norm(G[strict] - L[strict]) / ref_off if ref_off > 0 else 0.0
        d = np.arange(bar)
        diag = np.linalg.norm(G[d, d] - L[d, d]) / np.linalg.norm(L[d, d]) if bar else 0.0
        back = 0.0
        if bar:
            Gl = G[:, :bar]
            back = np.linalg.norm(A[:, :bar] - Gl @ Gl[:bar].T) / np.linalg.norm(A[:, :bar])
        schur = 0.0
        if bar < len(A):
            T = P[bar:, bar:]
            L21 = L[bar:, :bar]
            LL = L21 @ L21.T
            S_ref = A[bar:, bar:] - LL
            den = np.linalg.norm(A[bar:, bar:][T]) + np.linalg.norm(LL[T])
            schur = np.linalg.norm(G[bar:, bar:][T] - S_ref[T]) / den
        return {"lead_off": float(off), "lead_diag": float(diag), "lead_backward": float(back),
                "schur": float(schur)}

    def untouched(self, bar):
        """boolean mask of the trailing stored lower entries that no cross-cut product reaches
        (structurally |L21| |L21|^T == 0)"""
        P = self.pattern
        out = np.zeros_like(P)
        if 0 < bar < len(P):
            B21 = P[bar:, :bar].astype(np.float32)
            reach = (B21 @ B21.T) > 0
            out[bar:, bar:] = P[bar:, bar:] & ~reach
        elif bar == 0:
            out = P.copy()
        return out

    def check_partial(self, got, bar, what=""):
        """factorUpTo's result `got` (the solver's layout, in dtype): leading columns, Schur
        complement, and the untouched entries bitwise"""
        got = np.asarray(got)
        G = np.tril(self.sol.densify(got.astype(np.float64)))
        check(self.partial_errors_dense(G, bar), self.dtype, what)
        idx = data_index(self.sol)[self.untouched(bar)]
        assert bitwise_equal(got[idx], self.data[idx]), ("untouched entries changed", what,
                                                         int(np.count_nonzero(got[idx] != self.data[idx])))

    def trailing(self, bar):
        """the reference of factorFrom on data whose leading columns are not used: the float64
        Cholesky factor of A22 alone, as (L22, A22, pattern22)"""
        A22 = self.A[bar:, bar:]
        return np.linalg.cholesky(A22), A22, self.pattern[bar:, bar:]

    def check_trailing_factor(self, got, bar, what=""):
        """factorFrom(k) of data whose trailing block is A22: that block against the Cholesky of A22"""
        L22, A22, P22 = self.trailing(bar)
        G = np.tril(self.sol.densify(np.asarray(got, dtype=np.float64)))[bar:, bar:]
        G[~P22] = 0.0
        check(factor_errors_dense(G, L22, A22, P22), self.dtype, what)


def known_factor_data(sol, seed, dtype, rho=1.0, full_from=None):
    """a matrix A = L0 L0^T with L0 random on the stored pattern: diagonal uniform in [1, 2],
    off-diagonals uniform(-1, 1) * rho / sqrt(stored off-diagonal entries in the row).
    full_from=bar (a lump boundary): L0 random on the stored pattern of the columns < bar only, and on the
    columns >= bar nonzero only in the square diagonal blocks of the lumps (for solvers whose fill is
    incomplete past canFactorUpToSpan(): L0 L0^T must still lie on the stored pattern)"""
    dtype = np.dtype(dtype)
    n = sol.order()
    P = stored_pattern(sol)
    rng = np.random.default_rng(seed)
    strict = np.tril(P, -1)
    if full_from is not None:
        ls = sol.skel()["lumpStart"]
        lump_of = np.searchsorted(ls, np.arange(n), side="right") - 1
        same = lump_of[:, None] == lump_of[None, :]
        strict[:, full_from:] &= same[:, full_from:]
    per_row = np.maximum(strict.sum(axis=1), 1).astype(np.float64)
    L0 = np.where(strict, rng.uniform(-1.0, 1.0, size=(n, n)) * (rho / np.sqrt(per_row))[:, None], 0.0)
    L0[np.diag_indices(n)] = rng.uniform(1.0, 2.0, size=n)
    A0 = L0 @ L0.T
    outside = np.tril(~P)
    assert not np.any(A0[outside]), "L0 L0^T has entries outside the stored pattern (%d)" % \
        int(np.count_nonzero(A0[outside]))
    data = sparsify(sol, A0).astype(dtype)
    A = sol.densify(data.astype(np.float64), fill_upper_half=True)
    L = np.linalg.cholesky(A)
    return KnownFactor(sol, data, A, L, P)


def factor_errors_dense(G, L, A, pattern):
    strict = np.tril(pattern, -1)
    ref_off = np.linalg.norm(L[strict])
    off = np.linalg.norm(G[strict] - L[strict]) / ref_off if ref_off > 0 else 0.0
    diag = np.linalg.norm(np.diag(G) - np.diag(L)) / np.linalg.norm(np.diag(L))
    backward = np.linalg.norm(A - G @ G.T) / np.linalg.norm(A)
    return {"off": float(off), "diag": float(diag), "backward": float(backward)}


def solve_errors(M, b, x):
    """forward error against a float64 solve and normwise backward error ||b - M x|| / (||M|| ||x|| +
    ||b||), worst right-hand side of each (b, x: n x nRHS or n)"""
    b = np.asarray(b, dtype=np.float64).reshape(M.shape[0], -1)
    x = np.asarray(x, dtype=np.float64).reshape(M.shape[0], -1)
    ref = np.linalg.solve(M, b)
    fwd = np.linalg.norm(x - ref, axis=0) / np.linalg.norm(ref, axis=0)
    nM = np.linalg.norm(M)
    bwd = np.linalg.norm(b - M @ x, axis=0) / (nM * np.linalg.norm(x, axis=0) + np.linalg.norm(b, axis=0))
    return {"solve_forward": float(fwd.max()), "solve_backward": float(bwd.max())}


def ratios(errors, dtype):
    """every error over its tolerance"""
    return {k: v / tolerance(k, dtype) for k, v in errors.items()}


def check(errors, dtype, what=""):
    r = ratios(errors, dtype)
    bad = {k: (errors[k], tolerance(k, dtype)) for k, v in r.items() if not v < 1.0}
    assert not bad, ("known-factor check failed", what, np.dtype(dtype).name, bad)
    _record(r, dtype)


def vec_to_cols(v, n, nrhs):
    """a device-layout vector block (nRHS columns of stride n, column-major) as n x nRHS float64"""
    return np.asarray(v, dtype=np.float64).reshape(nrhs, n).T


# KNOWN_FACTOR_REPORT=<path>: the largest error / tolerance of the checks that passed, per dtype and
# metric, is written there as JSON when the process ends (how the constants above are judged against
# measured numbers)
_REPORT = os.environ.get("KNOWN_FACTOR_REPORT")
_worst = {}


def _record(r, dtype):
    if not _REPORT:
        return
    d = _worst.setdefault(np.dtype(dtype).name, {})
    for k, v in r.items():
        d[k] = max(d.get(k, 0.0), float(v))


@atexit.register
def _write_report():
    if _REPORT and _worst:
        with open(_REPORT, "w") as f:
            json.dump(_worst, f, indent=1, sort_keys=True)
