"""The driver of the device-resident Lanczos recurrence: the buffers of one run, the
bsp_lanczos_* pieces of a step and the chunked queue, and the host post-processing of the coefficients (Ritz
values, Gauss quadrature) in numpy.  sparse.lanczos, eig_extremes, cond2_estimate and logdet_slq are built on
it.  The scalars of the recurrence live in a state record on the device (12 words per matrix and start vector)
and are read by the kernels; the host reads the stop words once per chunk, or never."""
import ctypes

import numpy as np

from . import _call, _check, _ptr_arg, _ptr_of, _suffix

STOPS = ("running", "unused", "step limit", "invariant subspace", "non-finite", "zero start vector")
MAX_STEPS = 512  # of a run: the host post-processing is a dense eigen-solve of the tridiagonal


def _np_dtype(dtype):
    """the numpy dtype of a numpy or a torch dtype"""
    return np.dtype(str(dtype).replace("torch.", "")) if type(dtype).__module__.startswith("torch") else np.dtype(dtype)


def default_breakdown(dtype):
    """64 machine epsilons of the value type (a numpy dtype or a torch dtype)"""
    return 64.0 * float(np.finfo(_np_dtype(dtype)).eps)


def check_settings(what, steps, reorth, check_every=None, breakdown=None):
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError("%s: steps must be an integer >= 1, got %r" % (what, steps))
    if steps > MAX_STEPS:
        raise ValueError("%s: steps = %d; at most %d steps are taken in one run" % (what, steps, MAX_STEPS))
    if reorth not in ("full", None):
        raise ValueError("%s: reorth must be 'full' or None, got %r" % (what, reorth))
    if check_every is not None and (isinstance(check_every, bool) or not isinstance(check_every, int)
                                    or check_every < 1):
        raise ValueError("%s: check_every must be None or an integer >= 1, got %r" % (what, check_every))
    if breakdown is not None and (isinstance(breakdown, bool) or not isinstance(breakdown, (int, float))
                                  or not breakdown >= 0):
        raise ValueError("%s: breakdown must be None or a number >= 0, got %r" % (what, breakdown))


class LanczosRun:
    """One Lanczos run per (matrix, start vector) on the device.  v0: [n, q] or [B, n, q] (contiguous, device),
    the start vectors (normalised by the run).  apply_a(v, out) writes A v into out (both shaped like v0) and
    returns the tensor that holds it.  steps: kmax <= 512.  reorth "full": every w is orthogonalised twice
    against all earlier basis vectors (classical Gram-Schmidt), which keeps `steps` slots; None: the plain
    three-term recurrence on a ring of two slots (`steps` slots with keep_basis).  breakdown: a column stops on
    an invariant subspace when ww <= breakdown^2 (alpha^2 + beta_prev^2) (default 64 eps of the dtype).

    The records as device tensors: `state` int64 [.., q, 12], `coef` float64 [.., q, 2, steps] (alpha, beta; zero
    beyond the steps done), `basis` [slots, .., n, q] (slot j = v_j when the basis is kept).  Nothing here
    synchronises but running()."""

    def __init__(self, solver, v0, apply_a, steps, reorth="full", keep_basis=False, breakdown=None):
        import torch
        check_settings("LanczosRun", steps, reorth, None, breakdown)
        self.solver, self._lib = solver, solver._lib
        if v0.dim() not in (2, 3):
            raise ValueError("LanczosRun: v0 must be [n, q] or [B, n, q], got shape %s" % (tuple(v0.shape),))
        self.batched = v0.dim() == 3
        self.n, self.q = int(v0.shape[-2]), int(v0.shape[-1])
        self.nb = int(v0.shape[0]) if self.batched else 1
        self.sfx = _suffix(v0)
        _ptr_of(v0)
        self.v0, self.apply_a = v0, apply_a
        self.steps, self.full = int(steps), reorth == "full"
        self.kept = self.full or bool(keep_basis)
        self.slots = self.steps if self.kept else min(2, self.steps)
        self.breakdown = default_breakdown(v0.dtype) if breakdown is None else float(breakdown)
        lead = tuple(v0.shape[:-2])
        self.basis = torch.zeros((self.slots,) + tuple(v0.shape), dtype=v0.dtype, device=v0.device)
        self.w = torch.zeros_like(v0)
        self.state = torch.zeros(lead + (self.q, 12), dtype=torch.int64, device=v0.device)
        self.coef = torch.zeros(lead + (self.q, 2, self.steps), dtype=torch.float64, device=v0.device)
        need = ctypes.c_int64(0)
        self._head = (solver._h, ctypes.c_int64(self.n), ctypes.c_int64(self.q), ctypes.c_int64(self.steps))
        _check(self._lib.bsp_lanczos_work_bytes(*self._head, ctypes.byref(need)))
        self._work = torch.empty(need.value * self.nb + 16, dtype=torch.uint8, device=v0.device)
        self._tail = (ctypes.c_void_p((self._work.data_ptr() + 15) // 16 * 16), ctypes.c_void_p(_ptr_of(self.state)))
        self._count = (ctypes.c_int32(self.nb),) if self.batched else ()
        # slot s of member m is basis[s, m]: the member's array starts at basis[0, m], slots nb n q apart
        self._basis = (self._ptrs(self.basis[0]), ctypes.c_int64(self.nb * self.n * self.q), ctypes.c_int64(self.slots))
        self._w, self._coef = self._ptrs(self.w), ctypes.c_void_p(_ptr_of(self.coef))
        self.j = 0

    def _ptrs(self, t):
        return _ptr_arg(t.unbind(0) if self.batched else [t], self.batched)

    def _piece(self, name, vec, *args):
        _call(self._lib, "bsp_lanczos_" + name + "_", self.batched, self.sfx, *self._head, vec, *self._basis, *args,
              *self._tail, *self._count)

    def _slot(self, j):
        return j if self.kept else j % 2

    def start(self):
        """the records, vv and v_0"""
        self._piece("init", self._ptrs(self.v0), ctypes.c_int64(0), ctypes.c_double(self.breakdown))
        self.j = 0

    def iterate(self):
        """queues one step (nothing beyond `steps`)"""
        j = self.j
        if j >= self.steps:
            return
        i64, i32 = ctypes.c_int64, ctypes.c_int32
        w = self.apply_a(self.basis[self._slot(j)], self.w)
        if w is not self.w:
            self.w.copy_(w)
        self._piece("alpha", self._w, i64(self._slot(j)))
        self._piece("update", self._w, i64(self._slot(j)), i64(self._slot(max(j - 1, 0))), i32(0 if self.full else 1),
                    self._coef)
        if self.full:
            for last in (0, 1):
                self._piece("project", self._w, i64(j + 1))
                self._piece("subtract", self._w, i64(j + 1), i32(last), self._coef)
        if j + 1 < self.steps:
            self._piece("normalize", self._w, i64(self._slot(j + 1)))
        self.j = j + 1

    def running(self):
        """whether any problem still runs: one read of the device"""
        return bool((self.state[..., 1] == 0).any())

    def run(self, check_every=None):
        """start(), then `steps` steps queued in chunks of check_every, the stop words read once after each
        chunk (check_every None: one chunk, nothing read).  Stopped problems are frozen by the kernels, so the
        result does not depend on check_every."""
        self.start()
        while self.j < self.steps:
            k = self.steps - self.j if check_every is None else min(check_every, self.steps - self.j)
            for _ in range(k):
                self.iterate()
            if check_every is not None and self.j < self.steps and not self.running():
                break
        return self

    # ---- what the records say, as device tensors shaped [q] / [B, q] --------------------------------
    def steps_done(self):
        return self.state[..., 0].clone()

    def stop(self):
        return self.state[..., 1].clone()

    def alpha(self):
        return self.coef[..., 0, :]

    def beta(self):
        return self.coef[..., 1, :]


def read_state(t):
    """the state record(s) [.., 12] decoded on the host (this synchronises): a dict, or nested lists of them"""
    w = t.detach().cpu().numpy().astype(np.int64)
    if w.shape[-1] != 12:
        raise ValueError("read_state: expected an int64 tensor [.., 12], got shape %s" % (w.shape,))

    def decode(r):
        f = r.copy().view(np.float64)
        return {"steps": int(r[0]), "stop": int(r[1]), "stopReason": STOPS[int(r[1])], "vv": float(f[2]),
                "alpha": float(f[3]), "beta": float(f[4]), "ww": float(f[5]), "thr2": float(f[6]), "kmax": int(r[7])}

    def walk(a):
        return decode(a) if a.ndim == 1 else [walk(s) for s in a]

    return walk(w)


# ---- host post-processing of one column's coefficients (numpy only) -------------------------------------
def ritz(alpha, beta, k):
    """The Ritz values of k steps: (theta [k] ascending, tau [k], bound [k]) from the eigen-system T S = S
    diag(theta) of the k x k tridiagonal T = tridiag(beta_0 .. beta_{k-2}; alpha_0 .. alpha_{k-1}), by
    numpy.linalg.eigh: tau_i = s_{0,i}^2, the weights of the Gauss quadrature of the start vector's spectral
    measure, and bound_i = |beta_{k-1} s_{k-1,i}|, the residual |A y_i - theta_i y_i| of the Ritz vector: an
    eigenvalue of A lies within bound_i of theta_i."""
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > MAX_STEPS:
        raise ValueError("ritz: k must be an integer in [1, %d], got %r" % (MAX_STEPS, k))
    if alpha.ndim != 1 or beta.ndim != 1 or len(alpha) < k or len(beta) < k:
        raise ValueError("ritz: alpha and beta must hold at least k = %d coefficients, got %s and %s"
                         % (k, alpha.shape, beta.shape))
    k = int(k)
    T = np.diag(alpha[:k])
    if k > 1:
        T += np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)
    theta, S = np.linalg.eigh(T)
    return theta, S[0] ** 2, np.abs(beta[k - 1] * S[k - 1])


def quadrature(alpha, beta, k, f):
    """sum_i tau_i f(theta_i): the k-point Gauss quadrature of v^T f(A) v for the normalised start vector v"""
    theta, tau, _ = ritz(alpha, beta, k)
    return float(np.sum(tau * f(theta)))


def rademacher(n, q, seed, dtype=np.float64):
    """[n, q] probes of +-1 from numpy.random.default_rng(seed), on the host: the same seed gives the same probes"""
    return np.random.default_rng(seed).integers(0, 2, (n, q)).astype(_np_dtype(dtype)) * 2 - 1
