"""Differentiable sparse solve and log-determinant (torch.autograd) over a Solver's numeric layout.

    from baspacho_amd import autograd as BA
    x = BA.solve(solver, data, b)             # x = A(data)^-1 b
    ld = BA.logdet(solver, data)              # log det A(data)
    x, ld = BA.solve_logdet(solver, data, b)  # both, one factor

`data` is the solver's numeric layout, [dataSize] or a batch [B, dataSize] of matrices of one
structure; `b` is [n] or [n, k] (with a leading B when batched), in the solver's internal order, as
for Solver.solve.  A(data) is symmetric with A_ij = A_ji = data_e for every stored element e = (i, j),
i >= j; the strictly-upper elements of the diagonal blocks are not read and get gradient 0
(DESIGN.md section 13).  data's gradient is dense in the same layout: G_ij + G_ji off the diagonal,
G_ii on it, for the dense gradient G = df/dA.

Forward factors a clone of `data` (never modified).  Backward solves once more for b's gradient
(lambda = A^-1 g_x) and projects lambda x^T onto the pattern (Solver.patternGrad); the
log-determinant's gradient is A^-1 on the pattern, from a selected inversion of a clone of the saved
factor, run only when the log-determinant has a gradient.  All work is enqueued on
torch.cuda.current_stream(), nothing synchronises with the host, and the solver's own stream is
restored afterwards.  Double backward is not supported.

Through the factor itself:

    L = BA.cholesky(solver, data)             # the factor, in the same layout
    y = BA.solve_l(solver, L, b)              # y = L^-1 b
    x = BA.solve_lt(solver, L, b)             # x = L^-T b, e.g. a sample x = mu + L^-T z

cholesky returns L on the stored elements with i >= j and 0 on the strictly-upper elements of the
diagonal blocks; its backward is Solver.factorAdjoint on a clone of the incoming gradient (the
upper elements' gradient is ignored).  The half-solves' backward is one more half-solve and
Solver.patternOuter: Lbar = -(L^-T g_y) y^T and Lbar = -x (L^-1 g_x)^T, on the elements with i >= j.
"""
import torch
from torch.autograd.function import once_differentiable

__all__ = ["solve", "logdet", "solve_logdet", "cholesky", "solve_l", "solve_lt"]


class _OnCurrentStream:
    """run the solver on torch's current stream of `device`, then give it back its previous stream"""

    def __init__(self, solver, device):
        self.solver, self.device = solver, device

    def __enter__(self):
        self.prev = self.solver._stream
        self.solver.setStream(torch.cuda.current_stream(self.device))
        return self.solver

    def __exit__(self, *exc):
        self.solver.setStream(self.prev)
        return False


def _check_data(solver, data, what):
    if not isinstance(data, torch.Tensor):
        raise TypeError("%s: data must be a torch.Tensor, got %s" % (what, type(data).__name__))
    if data.dtype not in (torch.float64, torch.float32):
        raise TypeError("%s: data must be float64 or float32, got %s" % (what, data.dtype))
    if data.dim() not in (1, 2):
        raise ValueError("%s: data must be [dataSize] or [B, dataSize], got shape %s" % (what, tuple(data.shape)))
    if data.shape[-1] != solver.dataSize():
        raise ValueError("%s: data has %d elements per matrix, the solver's dataSize() is %d"
                         % (what, data.shape[-1], solver.dataSize()))
    if data.dim() == 2 and data.shape[0] == 0:
        raise ValueError("%s: empty batch" % what)


def _check_rhs(solver, data, b, what):
    if not isinstance(b, torch.Tensor):
        raise TypeError("%s: b must be a torch.Tensor, got %s" % (what, type(b).__name__))
    if b.dtype != data.dtype:
        raise TypeError("%s: b has dtype %s, data has %s" % (what, b.dtype, data.dtype))
    batched = data.dim() == 2
    lo = 2 if batched else 1
    if b.dim() not in (lo, lo + 1):
        raise ValueError("%s: b must be %s, got shape %s" % (
            what, "[B, n] or [B, n, k]" if batched else "[n] or [n, k]", tuple(b.shape)))
    if batched and b.shape[0] != data.shape[0]:
        raise ValueError("%s: batch sizes differ: data has %d matrices, b has %d" % (what, data.shape[0], b.shape[0]))
    n = b.shape[1] if batched else b.shape[0]
    if n != solver.order():
        raise ValueError("%s: b has %d rows, the solver's order() is %d" % (what, n, solver.order()))
    if b.dim() == lo + 1 and b.shape[-1] < 1:
        raise ValueError("%s: b has no right-hand sides" % what)


def _check_device(solver, what, *ts):
    for t in ts:
        if not t.is_cuda:
            raise ValueError("%s: tensors must live in device memory, got a %s tensor" % (what, t.device))
    if len({t.device for t in ts}) != 1:
        raise ValueError("%s: tensors on different devices: %s" % (what, sorted({str(t.device) for t in ts})))
    if solver.canFactorUpToSpan() < solver.numSpans():
        raise ValueError("%s: this solver can only factor up to span %d (AddFillForGivenElims); it needs a "
                         "complete factor" % (what, solver.canFactorUpToSpan()))


def _members(t):
    """the per-matrix tensors of a batched [B, ...] tensor, or [t] of a single one"""
    return list(t.unbind(0))


def _factor(solver, data):
    L = data.detach().clone(memory_format=torch.contiguous_format)
    solver.factor(_members(L) if L.dim() == 2 else L)
    return L


def _to_cols(v, batched):
    """b-shaped [.., n] / [.., n, k] -> a fresh contiguous [.., k, n]: solve()'s column-major layout"""
    vv = v.unsqueeze(-1) if v.dim() == (2 if batched else 1) else v
    out = torch.empty(vv.shape[:-2] + (vv.shape[-1], vv.shape[-2]), dtype=v.dtype, device=v.device)
    out.copy_(vv.transpose(-1, -2))
    return out


def _from_cols(xt, shape):
    """[.., k, n] -> b's shape ([.., n] or [.., n, k]), a view"""
    x = xt.transpose(-1, -2)
    return x.reshape(shape) if x.shape != shape else x


def _solve_cols(solver, L, xt):
    """xt <- A^-1 xt in place ([.., k, n])"""
    n, k = xt.shape[-1], xt.shape[-2]
    if L.dim() == 2:
        solver.solve(_members(L), _members(xt), stride=n, nRHS=k)
    else:
        solver.solve(L, xt, stride=n, nRHS=k)


def _backward(ctx, g_x, g_ld):
    """gradients (data, b) of the forward saved in ctx; g_x / g_ld None when that output is unused"""
    solver = ctx.solver
    L, xt = ctx.saved_tensors if ctx.has_x else (ctx.saved_tensors[0], None)
    batched = L.dim() == 2
    need_data, need_b = ctx.needs_input_grad[1], ctx.has_x and ctx.needs_input_grad[2]
    grad_data = grad_b = None
    with _OnCurrentStream(solver, L.device):
        lam = None
        if g_x is not None and (need_data or need_b):
            lam = _to_cols(g_x, batched)
            _solve_cols(solver, L, lam)
            if need_b:
                grad_b = _from_cols(lam, ctx.b_shape).clone()
        Z = scale = None
        if g_ld is not None and need_data:
            Z = L.clone()
            solver.selectedInverse(_members(Z) if batched else Z)
            scale = g_ld.reshape(-1).contiguous()
        if need_data and (Z is not None or lam is not None):
            grad_data = torch.empty_like(L)
            k = lam.shape[-2] if lam is not None else 1
            sel = _members if batched else (lambda t: t)
            solver.patternGrad(sel(grad_data), Z=None if Z is None else sel(Z), zScale=scale,
                               U=None if lam is None else sel(lam), V=None if lam is None else sel(xt),
                               nRHS=k, alpha=-1.0)
    return None, grad_data, grad_b


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, data, b):
        with _OnCurrentStream(solver, data.device):
            L = _factor(solver, data)
            xt = _to_cols(b.detach(), data.dim() == 2)
            _solve_cols(solver, L, xt)
        ctx.solver, ctx.has_x, ctx.b_shape = solver, True, b.shape
        ctx.save_for_backward(L, xt)
        ctx.set_materialize_grads(False)
        return _from_cols(xt, b.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x):
        return _backward(ctx, g_x, None)


class _LogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, data):
        with _OnCurrentStream(solver, data.device):
            L = _factor(solver, data)
            ld = solver.logDet(_members(L) if L.dim() == 2 else L)
        ctx.solver, ctx.has_x = solver, False
        ctx.save_for_backward(L)
        ctx.set_materialize_grads(False)
        return ld

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ld):
        return _backward(ctx, None, g_ld)[:2]


class _SolveLogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, data, b):
        with _OnCurrentStream(solver, data.device):
            L = _factor(solver, data)
            ld = solver.logDet(_members(L) if L.dim() == 2 else L)
            xt = _to_cols(b.detach(), data.dim() == 2)
            _solve_cols(solver, L, xt)
        ctx.solver, ctx.has_x, ctx.b_shape = solver, True, b.shape
        ctx.save_for_backward(L, xt)
        ctx.set_materialize_grads(False)
        return _from_cols(xt, b.shape), ld

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, g_ld):
        return _backward(ctx, g_x, g_ld)


def solve(solver, data, b):
    """x = A(data)^-1 b, differentiable in data and b (see the module docstring for the shapes)"""
    _check_data(solver, data, "solve")
    _check_rhs(solver, data, b, "solve")
    _check_device(solver, "solve", data, b)
    return _Solve.apply(solver, data, b)


def logdet(solver, data):
    """log det A(data): a 0-dim tensor, or [B] for a batch; differentiable in data"""
    _check_data(solver, data, "logdet")
    _check_device(solver, "logdet", data)
    return _LogDet.apply(solver, data)


def solve_logdet(solver, data, b):
    """(A(data)^-1 b, log det A(data)) from one factor: e.g. a Gaussian negative log-likelihood"""
    _check_data(solver, data, "solve_logdet")
    _check_rhs(solver, data, b, "solve_logdet")
    _check_device(solver, "solve_logdet", data, b)
    return _SolveLogDet.apply(solver, data, b)


# ---- through the factor: cholesky, solve_l, solve_lt ----------------------
def _upper_mask(solver, device):
    """bool device tensor [dataSize]: the strictly-upper elements of the diagonal blocks (cached)"""
    cache = solver.__dict__.setdefault("_upper_mask_dev", {})
    if device not in cache:
        cache[device] = torch.from_numpy(~solver.lowerMask()).to(device)
    return cache[device]


class _Cholesky(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, data):
        with _OnCurrentStream(solver, data.device):
            L = _factor(solver, data)
            L.masked_fill_(_upper_mask(solver, data.device), 0)
        ctx.solver = solver
        ctx.save_for_backward(L)
        ctx.set_materialize_grads(False)
        return L

    @staticmethod
    @once_differentiable
    def backward(ctx, g_L):
        if g_L is None or not ctx.needs_input_grad[1]:
            return None, None
        (L,) = ctx.saved_tensors
        solver = ctx.solver
        with _OnCurrentStream(solver, L.device):
            grad = g_L.clone(memory_format=torch.contiguous_format)
            if L.dim() == 2:
                solver.factorAdjoint(_members(L), _members(grad))
            else:
                solver.factorAdjoint(L, grad)
        return None, grad


def _half_solve(solver, name, L, vt):
    """vt <- L^-1 vt (name "solveL") or L^-T vt ("solveLt") in place ([.., k, n])"""
    n, k = vt.shape[-1], vt.shape[-2]
    if L.dim() == 2:
        getattr(solver, name)(_members(L), _members(vt), stride=n, nRHS=k)
    else:
        getattr(solver, name)(L, vt, stride=n, nRHS=k)


class _HalfSolve(torch.autograd.Function):
    """y = L^-1 b (lower = True) or x = L^-T b (lower = False)"""

    @staticmethod
    def forward(ctx, solver, L, b, lower):
        batched = L.dim() == 2
        with _OnCurrentStream(solver, L.device):
            L = L.detach().contiguous()
            yt = _to_cols(b.detach(), batched)
            _half_solve(solver, "solveL" if lower else "solveLt", L, yt)
        ctx.solver, ctx.lower, ctx.b_shape = solver, lower, b.shape
        ctx.save_for_backward(L, yt)
        ctx.set_materialize_grads(False)
        return _from_cols(yt, b.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y):
        if g_y is None:
            return None, None, None, None
        solver = ctx.solver
        L, yt = ctx.saved_tensors
        batched = L.dim() == 2
        need_L, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_L = grad_b = None
        if not (need_L or need_b):
            return None, None, None, None
        with _OnCurrentStream(solver, L.device):
            bt = _to_cols(g_y, batched)  # b's gradient: L^-T g_y (lower) or L^-1 g_x (upper)
            _half_solve(solver, "solveLt" if ctx.lower else "solveL", L, bt)
            if need_b:
                grad_b = _from_cols(bt, ctx.b_shape).clone()
            if need_L:
                grad_L = torch.empty_like(L)
                # Lbar = -bbar y^T (y = L^-1 b) or -x bbar^T (x = L^-T b), on the elements i >= j
                U, V = (bt, yt) if ctx.lower else (yt, bt)
                sel = _members if batched else (lambda t: t)
                solver.patternOuter(sel(grad_L), sel(U), sel(V), nRHS=bt.shape[-2], alpha=-1.0,
                                    stride=bt.shape[-1])
        return None, grad_L, grad_b, None


def cholesky(solver, data):
    """the factor L of A(data), in the solver's layout ([dataSize] or [B, dataSize]), differentiable in
    data.  The strictly-upper elements of the diagonal blocks are 0 and their gradient is ignored."""
    _check_data(solver, data, "cholesky")
    _check_device(solver, "cholesky", data)
    return _Cholesky.apply(solver, data)


def solve_l(solver, L, b):
    """y = L^-1 b for a factor L from cholesky(), differentiable in L and b (b as for solve)"""
    _check_data(solver, L, "solve_l")
    _check_rhs(solver, L, b, "solve_l")
    _check_device(solver, "solve_l", L, b)
    return _HalfSolve.apply(solver, L, b, True)


def solve_lt(solver, L, b):
    """x = L^-T b for a factor L from cholesky(), differentiable in L and b (b as for solve)"""
    _check_data(solver, L, "solve_lt")
    _check_rhs(solver, L, b, "solve_lt")
    _check_device(solver, "solve_lt", L, b)
    return _HalfSolve.apply(solver, L, b, False)
