"""The driver of the matrix-free least squares of DESIGN.md section 28: CGLS for (J^T J + D) x = J^T r + c from
the entries of J alone, on the lists of a JacobianProduct.  The buffers of one solve, the bsp_cgls_* pieces of
an iteration and the chunked queue, as cg.CgRun has them for the conjugate gradient; sparse.lstsq_cg is built
on it.  The state record is the conjugate gradient's (cg.read_state decodes it): rz = s.z, pAp = |J p|^2 + p^T
D p, rr = s.s, bb = |J^T r + c|^2, with s = J^T (r - J x) - D x + c the residual of the normal equations; the
residual r - J x itself is kept in m-space and updated there."""
import ctypes

from . import _call, _check, _ptr_arg, _ptr_of, _suffix
from .cg import MAX_BLOCK, STOPS, check_settings, read_state  # noqa: F401  (shared with the conjugate gradient)

PRECOND_KINDS = {"jacobi": 1, "block_jacobi": 2}


def _members(t, batched):
    return None if t is None else _ptr_arg(t.unbind(0) if batched else [t], batched)


def column_norms(product, values):
    """colsq [n] / [B, n], float64: the squared norms of the columns of J(values), each the fold over the column's
    entries in ascending entry index of double(v) * double(v) (bsp_cgls_colsq_*)"""
    import torch
    batched = values.dim() == 2
    out = torch.empty(tuple(values.shape[:-1]) + (product.n,), dtype=torch.float64, device=values.device)
    _call(product._lib, "bsp_cgls_colsq_", batched, _suffix(values), product.solver._h, product._h,
          _members(values, batched), _members(out, batched), *((ctypes.c_int32(values.shape[0]),) if batched else ()))
    return out


def damping_vector(product, colsq, alpha, beta, like):
    """d [n] / [B, n] of `like`'s dtype: d_i = alpha colsq_i + beta, taken in double (bsp_cgls_damp_*)"""
    import torch
    batched = colsq.dim() == 2
    out = torch.empty(colsq.shape, dtype=like.dtype, device=colsq.device)
    _call(product._lib, "bsp_cgls_damp_", batched, _suffix(like), product.solver._h, product._h,
          _members(colsq, batched), ctypes.c_double(float(alpha)), ctypes.c_double(float(beta)), _members(out, batched),
          *((ctypes.c_int32(colsq.shape[0]),) if batched else ()))
    return out


def _work(product, q, nb, device):
    import torch
    need = ctypes.c_int64(0)
    _check(product._lib.bsp_cgls_work_bytes(product.solver._h, product._h, ctypes.c_int64(q), ctypes.byref(need)))
    buf = torch.empty(need.value * nb + 16, dtype=torch.uint8, device=device)
    return buf, ctypes.c_void_p((buf.data_ptr() + 15) // 16 * 16)


class Preconditioner:
    """A built-in preconditioner (kind "jacobi" or "block_jacobi") of N = J^T J + D for the entry values [nnz] /
    [B, nnz] of the JacobianProduct `product`, built on the device (bsp_cgls_precond_build_*) from the column
    norms `colsq` (column_norms) and the damping vector `d` (damping_vector; None: no damping): `values` of the
    inverses and `status`, int64 [2] / [B, 2] = {the caller's scalar of the lowest bad pivot or -1, bad blocks}."""

    def __init__(self, product, kind, values, colsq, d):
        import torch
        if kind not in PRECOND_KINDS:
            raise ValueError("cgls: unknown built-in preconditioner %r" % (kind,))
        self.product, self.kind = product, PRECOND_KINDS[kind]
        batched = values.dim() == 2
        lead = tuple(values.shape[:-1])
        elems = product.precondInfo(kind)["inverse_elems"]
        self.values = torch.empty(lead + (max(elems, 1),), dtype=values.dtype, device=values.device)
        self.status = torch.empty(lead + (2,), dtype=torch.int64, device=values.device)
        nb = values.shape[0] if batched else 1
        self._buf, work = _work(product, 1, nb, values.device)
        _call(product._lib, "bsp_cgls_precond_build_", batched, _suffix(values), product.solver._h, product._h,
              ctypes.c_int32(self.kind), _members(values, batched), _members(colsq, batched), _members(d, batched),
              _members(self.values, batched), work, ctypes.c_void_p(_ptr_of(self.status)),
              *((ctypes.c_int32(nb),) if batched else ()))


class CglsRun:
    """One CGLS solve on the device.  values: [nnz] / [B, nnz]; r: [m, q] / [B, m, q] or None; c: [n, q] / [B, n, q]
    or None (not both None); d: the damping vector [n] / [B, n] or None; x: [n, q] / [B, n, q], the start when
    `has_x0` (else it must hold zeros), overwritten by the iterates.  All contiguous, on the device, of one dtype.
    precond: None, a Preconditioner, or a callable s -> z on tensors shaped like x.  Nothing here synchronises but
    running()."""

    def __init__(self, product, values, r, c, d, x, has_x0, precond, tol, max_steps):
        import torch
        if r is None and c is None:
            raise ValueError("cgls: r and c cannot both be absent")
        self.product, self.solver, self._lib = product, product.solver, product._lib
        self.batched = values.dim() == 2
        self.n, self.m, self.q = product.n, product.m, int(x.shape[-1])
        self.nb = int(values.shape[0]) if self.batched else 1
        self.sfx = _suffix(values)
        for t in (values, r, c, d, x):
            if t is not None:
                _ptr_of(t)
        self.values, self.r, self.c, self.d, self.x, self.has_x0 = values, r, c, d, x, has_x0
        self.precond = precond
        self.built_in = isinstance(precond, Preconditioner)
        lead = tuple(x.shape[:-2])
        mshape = lead + (self.m, self.q)
        self.res = torch.zeros(mshape, dtype=x.dtype, device=x.device) if r is None or has_x0 else r.clone()
        self.t = torch.zeros(mshape, dtype=x.dtype, device=x.device)
        self.s = torch.zeros_like(x)
        self.p = torch.zeros_like(x)
        self.z = torch.zeros_like(x) if self.built_in else None
        self.state = torch.zeros(lead + (self.q, 12), dtype=torch.int64, device=x.device)
        self._buf, self._work = _work(product, self.q, self.nb, x.device)
        self._state = ctypes.c_void_p(_ptr_of(self.state))
        self._count = (ctypes.c_int32(self.nb),) if self.batched else ()
        self._q = ctypes.c_int64(self.q)
        self._fixed = {}
        self.tol, self.max_steps = float(tol), int(max_steps)

    def _ptrs(self, t):
        return _members(t, self.batched)

    def _args(self, key, *tensors):
        """the pointer arguments of tensors that never move, built once"""
        if key not in self._fixed:
            self._fixed[key] = tuple(self._ptrs(t) for t in tensors)
        return self._fixed[key]

    def _piece(self, name, *args):
        _call(self._lib, "bsp_cgls_" + name + "_", self.batched, self.sfx, self.solver._h, self.product._h, *args,
              *self._count)

    def _normal(self, with_x, state):
        """s = J^T res - D x + c (with_x False: b = J^T r + c into s)"""
        if with_x:
            a = self._args("normal", self.values, self.res, self.d, self.x if self.d is not None else None, self.c, self.s)
        else:
            a = self._args("b", self.values, self.r, None, None, self.c, self.s)
        self._piece("normal", *a[:5], self._q, a[5], state)

    def _callable_z(self):
        """z = M^-1 s of the caller's preconditioner, checked"""
        z = self.precond(self.s)
        if not hasattr(z, "shape") or z.shape != self.s.shape or z.dtype != self.s.dtype or z.device != self.s.device:
            raise ValueError("cgls: the preconditioner must return a %s tensor of shape %s on %s"
                             % (self.s.dtype, tuple(self.s.shape), self.s.device))
        return z.contiguous()

    def _apply(self, start):
        """z = M^-1 s, ss, the stop test, gamma and beta; returns the tensor that holds z"""
        flag = ctypes.c_int32(1 if start else 0)
        if self.built_in:
            pc = self.precond
            mi, s, z = self._args("apply", pc.values, self.s, self.z)
            self._piece("apply", ctypes.c_int32(pc.kind), self._q, mi, s, z, flag, self._work, self._state)
            return self.z
        if self.precond is None:
            z = self.s
            zp = self._args("s", self.s)[0]
        else:
            z = self._callable_z()
            zp = self._ptrs(z)
        self._piece("apply", ctypes.c_int32(0), self._q, None, self._args("s", self.s)[0], zp, flag, self._work,
                    self._state)
        return z

    def _direction(self, z):
        zp = self._args("zdir", z)[0] if z is self.z or z is self.s else self._ptrs(z)
        _call(self._lib, "bsp_cg_direction_", self.batched, self.sfx, self.solver._h, ctypes.c_int64(self.n), self._q,
              zp, self._args("p", self.p)[0], ctypes.c_int32(1 if self.precond is None else 0), self._work,
              self._state, *self._count)

    def start(self):
        """b, the records, the first residuals and the first direction"""
        if self.r is not None:
            self._normal(False, None)
        else:
            self.s.copy_(self.c)
        self._piece("init", self._q, *self._args("init", self.s, self.x), ctypes.c_double(self.tol),
                    ctypes.c_int64(self.max_steps), self._work, self._state)
        if self.has_x0:
            self._piece("residual", *self._args("res0", self.values, self.x, self.r), self._q,
                        self._args("res", self.res)[0], self._state)
            self._normal(True, self._state)
        self._direction(self._apply(True))

    def iterate(self):
        """queues one iteration: one call of the C ABI (two around a callable preconditioner)"""
        if "iterate" not in self._fixed:
            pc = self.precond if self.built_in else None
            z = self.z if self.built_in else self.s
            self._fixed["iterate"] = (ctypes.c_int32(pc.kind if pc else 0),) + tuple(self._ptrs(t) for t in (
                self.values, self.d, self.c, pc.values if pc else None, self.p, self.t, self.x, self.res, self.s, z))
        kind, v, d, c, mi, p, t, x, res, s, z = self._fixed["iterate"]
        tail = (self._work, self._state)
        if self.built_in or self.precond is None:
            self._piece("iterate", kind, ctypes.c_int32(0), self._q, v, d, c, mi, p, t, x, res, s, z, *tail)
            return
        self._piece("iterate", kind, ctypes.c_int32(1), self._q, v, d, c, None, p, t, x, res, s, None, *tail)
        zc = self._callable_z()
        self._piece("iterate", kind, ctypes.c_int32(2), self._q, None, None, None, None, p, None, None, None, s,
                    self._ptrs(zc), *tail)

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
        """sqrt(rr / bb) of the recurrence residual of the normal equations (0 for a zero right-hand side)"""
        import torch
        f = self.state.view(torch.float64)
        rel = torch.sqrt(f[..., 4] / f[..., 5])
        return torch.where(self.state[..., 1] == 5, torch.zeros_like(rel), rel)
