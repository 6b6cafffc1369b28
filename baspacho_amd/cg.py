"""The driver of the device-resident preconditioned conjugate gradient: the buffers
of one solve, the bsp_cg_* pieces of an iteration and the chunked queue.  sparse.solve_cg and pcg.DevicePCG
are built on it.  The scalars of the iteration live in a state record on the device (12 words per matrix
and right-hand side) and are read by the kernels; the host reads the stop words once per chunk, or never."""
import ctypes

import numpy as np

from . import _call, _check, _ptr_arg, _ptr_of, _suffix

STOPS = ("running", "converged", "step limit", "breakdown", "non-finite", "zero right-hand side")
PRECOND_KINDS = {"jacobi": 1, "block_jacobi": 2, "fsai": 3}
FSAI = PRECOND_KINDS["fsai"]
MAX_BLOCK = 32  # widest param of block_jacobi


def check_settings(what, tol, max_steps, check_every):
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not tol >= 0:
        raise ValueError("%s: tol must be a number >= 0, got %r" % (what, tol))
    if isinstance(max_steps, bool) or not isinstance(max_steps, int) or max_steps < 0:
        raise ValueError("%s: max_steps must be an integer >= 0, got %r" % (what, max_steps))
    if check_every is not None and (isinstance(check_every, bool) or not isinstance(check_every, int)
                                    or check_every < 1):
        raise ValueError("%s: check_every must be None or an integer >= 1, got %r" % (what, check_every))


class Preconditioner:
    """A built-in preconditioner (kind "jacobi", "block_jacobi" or "fsai") of the SymProduct `product` for the
    entry values [nnz] / [B, nnz], built on the device (bsp_cg_precond_build_*): `values` of the inverses (of
    the sparse factor G of the approximate inverse G^T G for "fsai"), and `status`, int64
    [2] / [B, 2] = {the caller's scalar of the lowest bad pivot or -1, bad blocks (rows of G for "fsai")}."""

    def __init__(self, product, kind, values):
        import torch
        if kind not in PRECOND_KINDS:
            raise ValueError("cg: unknown built-in preconditioner %r" % (kind,))
        self.product, self.kind = product, PRECOND_KINDS[kind]
        sol, lib = product.solver, product._lib
        info = (ctypes.c_int64 * 4)()
        _check(lib.bsp_cg_precond_info(product._h, ctypes.c_int32(self.kind), info))
        batched = values.dim() == 2
        lead = tuple(values.shape[:-1])
        self.values = torch.empty(lead + (max(int(info[2]), 1),), dtype=values.dtype, device=values.device)
        self.status = torch.empty(lead + (2,), dtype=torch.int64, device=values.device)
        need = ctypes.c_int64(0)
        _check(lib.bsp_cg_work_bytes(sol._h, ctypes.c_int64(product.n), ctypes.c_int64(1), ctypes.byref(need)))
        nb = values.shape[0] if batched else 1
        work = torch.empty(need.value * nb + 16, dtype=torch.uint8, device=values.device)
        members = lambda t: t.unbind(0) if batched else [t]
        _call(lib, "bsp_cg_precond_build_", batched, _suffix(values), sol._h, product._h, ctypes.c_int32(self.kind),
              _ptr_arg(members(values), batched), _ptr_arg(members(self.values), batched),
              ctypes.c_void_p((work.data_ptr() + 15) // 16 * 16), ctypes.c_void_p(_ptr_of(self.status)),
              *((ctypes.c_int32(nb),) if batched else ()))


class CgRun:
    """One conjugate-gradient solve on the device.  b: [n, q] or [B, n, q] (contiguous, device); x: a tensor of
    b's shape holding the start, overwritten by the iterates; r: b - A x for that start.  apply_a(p, ap) writes
    A p into ap (both shaped like b).  precond: None (plain CG), a Preconditioner, or a callable r -> z on
    tensors shaped like b.  Nothing here synchronises but running()."""

    def __init__(self, solver, b, x, r, apply_a, precond, tol, max_steps):
        import torch
        self.solver, self._lib = solver, solver._lib
        self.batched = b.dim() == 3
        self.n, self.q = int(b.shape[-2]), int(b.shape[-1])
        self.nb = int(b.shape[0]) if self.batched else 1
        self.sfx = _suffix(b)
        for t in (b, x, r):
            _ptr_of(t)
        self.b, self.x, self.r = b, x, r
        self.apply_a, self.precond = apply_a, precond
        self.plain = precond is None
        # (a preconditioner with a cg_apply(run) of its own, as the reduced system's of sparse.lstsq_cg, is built-in too)
        self.built_in = isinstance(precond, Preconditioner) or hasattr(precond, "cg_apply")
        self.p = torch.zeros_like(b)
        self.ap = torch.zeros_like(b)
        self.z = torch.zeros_like(b) if self.built_in else None
        self.t = torch.zeros_like(b) if self.built_in and precond.kind == FSAI else None  # scratch: t = G r
        lead = tuple(b.shape[:-2])
        self.state = torch.zeros(lead + (self.q, 12), dtype=torch.int64, device=b.device)
        need = ctypes.c_int64(0)
        _check(self._lib.bsp_cg_work_bytes(solver._h, ctypes.c_int64(self.n), ctypes.c_int64(self.q),
                                           ctypes.byref(need)))
        self._work = torch.empty(need.value * self.nb + 16, dtype=torch.uint8, device=b.device)
        self._tail = (ctypes.c_void_p((self._work.data_ptr() + 15) // 16 * 16), ctypes.c_void_p(_ptr_of(self.state)))
        self._count = (ctypes.c_int32(self.nb),) if self.batched else ()
        self._nq = (ctypes.c_int64(self.n), ctypes.c_int64(self.q))
        self._plain = ctypes.c_int32(1 if self.plain else 0)
        self._fixed = {}
        self.tol, self.max_steps = float(tol), int(max_steps)

    def _ptrs(self, t):
        return _ptr_arg(t.unbind(0) if self.batched else [t], self.batched)

    def _piece(self, name, *args):
        _call(self._lib, "bsp_cg_" + name + "_", self.batched, self.sfx, self.solver._h, *args, *self._tail,
              *self._count)

    def _args(self, key, *tensors):
        """the pointer arguments of tensors that never move, built once"""
        if key not in self._fixed:
            self._fixed[key] = tuple(self._ptrs(t) for t in tensors)
        return self._fixed[key]

    def _apply_precond(self):
        """z = M^-1 r, rz and beta; returns the tensor that holds z"""
        if self.built_in:
            pc = self.precond
            if hasattr(pc, "cg_apply"):
                pc.cg_apply(self)
                return self.z
            if pc.kind == FSAI:
                _call(self._lib, "bsp_fsai_apply_", self.batched, self.sfx, self.solver._h, pc.product._h, *self._nq,
                      *self._args("fsai", pc.values, self.r, self.t, self.z), *self._tail, *self._count)
                return self.z
            self._piece("precond", pc.product._h, ctypes.c_int32(pc.kind), *self._nq,
                        *self._args("precond", pc.values, self.r, self.z))
            return self.z
        z = self.precond(self.r)
        if not hasattr(z, "shape") or z.shape != self.r.shape or z.dtype != self.r.dtype or z.device != self.r.device:
            raise ValueError("cg: the preconditioner must return a %s tensor of shape %s on %s"
                             % (self.r.dtype, tuple(self.r.shape), self.r.device))
        z = z.contiguous()
        self._piece("precond", None, ctypes.c_int32(0), *self._nq, None, self._args("r", self.r)[0], self._ptrs(z))
        return z

    def _direction(self, z):
        if z is self.z or z is self.r:
            zp = self._args("zdir", z)[0]
        else:
            zp = self._ptrs(z)
        self._piece("direction", *self._nq, zp, self._args("p", self.p)[0], self._plain)

    def start(self):
        """the records, bb, rr and the first direction"""
        self._piece("init", *self._nq, *self._args("init", self.b, self.x, self.r), ctypes.c_double(self.tol),
                    ctypes.c_int64(self.max_steps), self._plain)
        self._direction(self.r if self.plain else self._apply_precond())

    def iterate(self):
        """queues one iteration"""
        ap = self.apply_a(self.p, self.ap)
        if ap is self.ap:
            pa = self._args("alpha", self.p, self.ap)
        else:
            ap = ap.contiguous()
            pa = (self._args("p", self.p)[0], self._ptrs(ap))
        self._piece("alpha", *self._nq, *pa)
        self._piece("update", *self._nq, *pa, *self._args("xr", self.x, self.r), self._plain)
        self._direction(self.r if self.plain else self._apply_precond())

    def running(self):
        """whether any problem still runs: one read of the device"""
        return bool((self.state[..., 1] == 0).any())

    def run(self, check_every):
        """start(), then max_steps iterations queued in chunks of check_every, the stop words read once after
        each chunk (check_every None: one chunk, nothing read).  Stopped problems are frozen by the kernels, so
        the result does not depend on check_every."""
        self.start()
        done = 0
        while done < self.max_steps:
            k = self.max_steps - done if check_every is None else min(check_every, self.max_steps - done)
            for _ in range(k):
                self.iterate()
            done += k
            if check_every is not None and done < self.max_steps and not self.running():
                break
        return self

    # ---- what the records say, as device tensors shaped [q] / [B, q] --------------------------------
    def iterations(self):
        return self.state[..., 0].clone()

    def stop(self):
        return self.state[..., 1].clone()

    def relres(self):
        """sqrt(rr / bb) of the recurrence residual (NaN for a zero right-hand side's 0 / 0 is replaced by 0)"""
        import torch
        f = self.state.view(torch.float64)
        rel = torch.sqrt(f[..., 4] / f[..., 5])
        return torch.where(self.state[..., 1] == 5, torch.zeros_like(rel), rel)


def read_state(t):
    """the state record(s) [.., 12] decoded on the host (this synchronises): a dict, or nested lists of them"""
    w = t.detach().cpu().numpy().astype(np.int64)
    if w.shape[-1] != 12:
        raise ValueError("read_state: expected an int64 tensor [.., 12], got shape %s" % (w.shape,))

    def decode(r):
        f = r.copy().view(np.float64)
        return {"iterations": int(r[0]), "stop": int(r[1]), "stopReason": STOPS[int(r[1])], "rz": float(f[2]),
                "pAp": float(f[3]), "rr": float(f[4]), "bb": float(f[5]), "alpha": float(f[6]), "beta": float(f[7]),
                "tol2": float(f[8]), "maxSteps": int(r[9])}

    def walk(a):
        return decode(a) if a.ndim == 1 else [walk(s) for s in a]

    return walk(w)
