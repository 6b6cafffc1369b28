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

Products with the factor, the inverse maps of the half-solves:

    y = BA.mul_l(solver, L, x)                # y = L x, e.g. a sample x = mu + L z with covariance A
    w = BA.mul_lt(solver, L, x)               # w = L^T x, e.g. the whitened residual L^T (x - mu)

Their backward is the other product (xbar = L^T ybar, xbar = L ybar) and Solver.patternOuter: Lbar = ybar x^T
and Lbar = x ybar^T, on the elements with i >= j.

Through selected inversion:

    Z = BA.selected_inverse(solver, L)        # A^-1 on the pattern of L, for a factor L from cholesky()

Z is what Solver.selectedInverse writes: every slot of the layout, the diagonal blocks full and symmetric.
Its backward is Solver.selectedInverseAdjoint on a clone of the incoming gradient (every slot counts, the
strictly-upper ones as weights of Z_ji); the gradient of L is 0 on the strictly-upper elements.  The
sweep adds with float atomics: gradients are close, not bitwise, from run to run.

Through the partial factor, `span` a span that Solver.factorUpTo accepts:

    P = BA.factor_up_to(solver, data, span)        # [L11 0; L21 S] in the layout
    S = BA.schur_complement(solver, data, span)    # dense S = A22 - A21 A11^-1 A12, [m, m], internal order
    y = BA.solve_l_up_to(solver, P, span, b)       # [L11 0; L21 I]^-1 b; y[bar:] = b2 - A21 A11^-1 b1

Backward is Solver.factorAdjointUpTo (for schur_complement after Solver.schurComplementAdjoint, in one
Function); solve_l_up_to's is Solver.solveLtUpTo and Solver.patternOuter with y zeroed behind the cut.
"""
import torch
from torch.autograd.function import once_differentiable

__all__ = ["solve", "logdet", "solve_logdet", "cholesky", "solve_l", "solve_lt", "selected_inverse", "factor_up_to",
           "schur_complement", "solve_l_up_to", "mul_l", "mul_lt"]


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


# ---- products with the factor: mul_l, mul_lt ---------------------------------
def _product(solver, lower, L, vt):
    """a fresh L vt (lower) or L^T vt ([.., k, n])"""
    n, k = vt.shape[-1], vt.shape[-2]
    sel = _members if L.dim() == 2 else (lambda t: t)
    out = torch.empty_like(vt)
    (solver.mulL if lower else solver.mulLt)(sel(L), sel(vt), out=sel(out), stride=n, nRHS=k)
    return out


class _FactorProduct(torch.autograd.Function):
    """y = L x (lower = True) or y = L^T x (lower = False)"""

    @staticmethod
    def forward(ctx, solver, L, x, lower):
        batched = L.dim() == 2
        with _OnCurrentStream(solver, L.device):
            L = L.detach().contiguous()
            xt = _to_cols(x.detach(), batched)
            yt = _product(solver, lower, L, xt)
        ctx.solver, ctx.lower, ctx.x_shape = solver, lower, x.shape
        ctx.save_for_backward(L, xt)
        ctx.set_materialize_grads(False)
        return _from_cols(yt, x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y):
        if g_y is None:
            return None, None, None, None
        solver = ctx.solver
        L, xt = ctx.saved_tensors
        batched = L.dim() == 2
        need_L, need_x = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_L = grad_x = None
        if not (need_L or need_x):
            return None, None, None, None
        with _OnCurrentStream(solver, L.device):
            gt = _to_cols(g_y, batched)
            if need_x:  # xbar = L^T ybar (y = L x) or L ybar (y = L^T x)
                grad_x = _from_cols(_product(solver, not ctx.lower, L, gt), ctx.x_shape)
            if need_L:
                grad_L = torch.empty_like(L)
                # Lbar = ybar x^T (y = L x) or x ybar^T (y = L^T x), on the elements i >= j
                U, V = (gt, xt) if ctx.lower else (xt, gt)
                sel = _members if batched else (lambda t: t)
                solver.patternOuter(sel(grad_L), sel(U), sel(V), nRHS=gt.shape[-2], alpha=1.0, stride=gt.shape[-1])
        return None, grad_L, grad_x, None


def mul_l(solver, L, x):
    """y = L x for L in the solver's layout (the elements i >= j; e.g. from cholesky()), differentiable in
    L and x (x as b for solve)"""
    _check_data(solver, L, "mul_l")
    _check_rhs(solver, L, x, "mul_l")
    _check_device(solver, "mul_l", L, x)
    return _FactorProduct.apply(solver, L, x, True)


def mul_lt(solver, L, x):
    """y = L^T x for L in the solver's layout (the elements i >= j; e.g. from cholesky()), differentiable
    in L and x (x as b for solve), e.g. the whitened residual w = L^T (x - mu)"""
    _check_data(solver, L, "mul_lt")
    _check_rhs(solver, L, x, "mul_lt")
    _check_device(solver, "mul_lt", L, x)
    return _FactorProduct.apply(solver, L, x, False)


# ---- through selected inversion ----------------------------------------------
class _SelectedInverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, L):
        sel = _members if L.dim() == 2 else (lambda t: t)
        with _OnCurrentStream(solver, L.device):
            L = L.detach().contiguous()
            Z = L.clone()
            solver.selectedInverse(sel(Z))
        ctx.solver = solver
        ctx.save_for_backward(L, Z)
        ctx.set_materialize_grads(False)
        return Z

    @staticmethod
    @once_differentiable
    def backward(ctx, g_Z):
        if g_Z is None or not ctx.needs_input_grad[1]:
            return None, None
        L, Z = ctx.saved_tensors
        solver = ctx.solver
        sel = _members if L.dim() == 2 else (lambda t: t)
        with _OnCurrentStream(solver, L.device):
            grad = g_Z.clone(memory_format=torch.contiguous_format)
            solver.selectedInverseAdjoint(sel(L), sel(Z), sel(grad))
        return None, grad


def selected_inverse(solver, L):
    """Z = A^-1 on the pattern of L = cholesky(solver, data), in the solver's layout ([dataSize] or
    [B, dataSize]; diagonal blocks full and symmetric), differentiable in L.  Every slot of Z takes a
    gradient; L's gradient is 0 on the strictly-upper elements of the diagonal blocks."""
    _check_data(solver, L, "selected_inverse")
    _check_device(solver, "selected_inverse", L)
    return _SelectedInverse.apply(solver, L)


# ---- through the partial factor: factor_up_to, schur_complement, solve_l_up_to ----
def _check_span(solver, span, what):
    """the first scalar behind the cut; refuses what Solver.factorUpTo refuses (host-side, from the skeleton)"""
    if not isinstance(span, int) or not 0 <= span <= solver.numSpans():
        raise ValueError("%s: span must be an int in [0, %d], got %r" % (what, solver.numSpans(), span))
    sk = solver.skel()
    if int(sk["spanOffsetInLump"][span]) != 0:
        raise ValueError("%s: span %d lies inside a lump" % (what, span))
    lump = int(sk["spanToLump"][span])
    rs = [int(r) for r in solver.sparseEliminationRanges()]
    for a, b in zip(rs[:-1], rs[1:]):
        if a < lump < b:
            raise ValueError("%s: span %d cuts the sparse-elimination range [%d, %d)" % (what, span, a, b))
    return int(sk["spanStart"][span])


def _check_dest(solver, data, bar, dest, what):
    if dest is None:
        return
    m = solver.order() - bar
    if not isinstance(dest, torch.Tensor) or dest.dtype != torch.int32 or dest.shape != (m,) \
            or dest.device != data.device or not dest.is_contiguous():
        raise ValueError("%s: dest must be a contiguous int32 tensor [%d] on %s" % (what, m, data.device))


def _factor_up_to(solver, data, span):
    P = data.detach().clone(memory_format=torch.contiguous_format)
    solver.factorUpTo(_members(P) if P.dim() == 2 else P, span)
    P.masked_fill_(_upper_mask(solver, data.device), 0)
    return P


class _FactorUpTo(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, data, span):
        with _OnCurrentStream(solver, data.device):
            P = _factor_up_to(solver, data, span)
        ctx.solver, ctx.span = solver, span
        ctx.save_for_backward(P)
        ctx.set_materialize_grads(False)
        return P

    @staticmethod
    @once_differentiable
    def backward(ctx, g_P):
        if g_P is None or not ctx.needs_input_grad[1]:
            return None, None, None
        (P,) = ctx.saved_tensors
        solver = ctx.solver
        with _OnCurrentStream(solver, P.device):
            grad = g_P.clone(memory_format=torch.contiguous_format)
            sel = _members if P.dim() == 2 else (lambda t: t)
            solver.factorAdjointUpTo(sel(P), sel(grad), ctx.span)
        return None, grad, None


class _SchurComplement(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, data, span, dest):
        batched = data.dim() == 2
        sel = _members if batched else (lambda t: t)
        with _OnCurrentStream(solver, data.device):
            P = _factor_up_to(solver, data, span)
            m = solver._schurOrder(span)
            S = torch.empty(data.shape[:-1] + (m, m), dtype=data.dtype, device=data.device)
            solver.schurComplement(sel(P), span, out=sel(S), dest=dest)
        ctx.solver, ctx.span, ctx.dest = solver, span, dest
        ctx.save_for_backward(P)
        ctx.set_materialize_grads(False)
        return S

    @staticmethod
    @once_differentiable
    def backward(ctx, g_S):
        if g_S is None or not ctx.needs_input_grad[1]:
            return None, None, None, None
        (P,) = ctx.saved_tensors
        solver = ctx.solver
        sel = _members if P.dim() == 2 else (lambda t: t)
        with _OnCurrentStream(solver, P.device):
            grad = torch.empty_like(P)  # written whole by the adjoint of the extraction
            solver.schurComplementAdjoint(sel(g_S.contiguous()), ctx.span, out=sel(grad), dest=ctx.dest)
            solver.factorAdjointUpTo(sel(P), sel(grad), ctx.span)
        return None, grad, None, None


class _SchurOfFactor(torch.autograd.Function):
    """the dense trailing block of a partial factor P (for callers that also need P itself)"""

    @staticmethod
    def forward(ctx, solver, P, span, dest):
        sel = _members if P.dim() == 2 else (lambda t: t)
        m = solver._schurOrder(span)
        with _OnCurrentStream(solver, P.device):
            S = torch.empty(P.shape[:-1] + (m, m), dtype=P.dtype, device=P.device)
            solver.schurComplement(sel(P.detach().contiguous()), span, out=sel(S), dest=dest)
        ctx.solver, ctx.span, ctx.dest, ctx.shape = solver, span, dest, P.shape
        ctx.set_materialize_grads(False)
        return S

    @staticmethod
    @once_differentiable
    def backward(ctx, g_S):
        if g_S is None or not ctx.needs_input_grad[1]:
            return None, None, None, None
        solver = ctx.solver
        sel = _members if len(ctx.shape) == 2 else (lambda t: t)
        with _OnCurrentStream(solver, g_S.device):
            grad = torch.empty(ctx.shape, dtype=g_S.dtype, device=g_S.device)
            solver.schurComplementAdjoint(sel(g_S.contiguous()), ctx.span, out=sel(grad), dest=ctx.dest)
        return None, grad, None, None


class _SolveLUpTo(torch.autograd.Function):
    """y = M^-1 b, M = [L11 0; L21 I] of the partial factor P"""

    @staticmethod
    def forward(ctx, solver, P, span, bar, b):
        batched = P.dim() == 2
        sel = _members if batched else (lambda t: t)
        with _OnCurrentStream(solver, P.device):
            P = P.detach().contiguous()
            yt = _to_cols(b.detach(), batched)
            solver.solveLUpTo(sel(P), span, sel(yt), stride=yt.shape[-1], nRHS=yt.shape[-2])
        ctx.solver, ctx.span, ctx.bar, ctx.b_shape = solver, span, bar, b.shape
        ctx.save_for_backward(P, yt)
        ctx.set_materialize_grads(False)
        return _from_cols(yt, b.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y):
        need_P, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[4]
        if g_y is None or not (need_P or need_b):
            return None, None, None, None, None
        solver = ctx.solver
        P, yt = ctx.saved_tensors
        batched = P.dim() == 2
        sel = _members if batched else (lambda t: t)
        grad_P = grad_b = None
        with _OnCurrentStream(solver, P.device):
            bt = _to_cols(g_y, batched)  # b's gradient: M^-T g_y
            solver.solveLtUpTo(sel(P), ctx.span, sel(bt), stride=bt.shape[-1], nRHS=bt.shape[-2])
            if need_b:
                grad_b = _from_cols(bt, ctx.b_shape).clone()
            if need_P:
                # Pbar = -bbar y0^T on i >= j, y0 = y zeroed behind the cut: M does not depend on the
                # columns behind it, which get exactly 0
                y0 = yt.clone()
                y0[..., ctx.bar:] = 0
                grad_P = torch.empty_like(P)
                solver.patternOuter(sel(grad_P), sel(bt), sel(y0), nRHS=bt.shape[-2], alpha=-1.0,
                                    stride=bt.shape[-1])
        return None, grad_P, None, None, grad_b


def factor_up_to(solver, data, span):
    """the partial factor P = [L11 0; L21 S] of A(data) up to `span` (Solver.factorUpTo), in the solver's
    layout ([dataSize] or [B, dataSize]), differentiable in data.  The strictly-upper elements of the
    diagonal blocks are 0 and their gradient is ignored."""
    _check_data(solver, data, "factor_up_to")
    _check_device(solver, "factor_up_to", data)
    _check_span(solver, span, "factor_up_to")
    return _FactorUpTo.apply(solver, data, span)


def schur_complement(solver, data, span, dest=None):
    """the Schur complement S = A22 - A21 A11^-1 A12 of A(data) on the spans from `span` on, dense and
    symmetric, [m, m] or [B, m, m], differentiable in data.  Rows and columns in the solver's internal
    order, or at dest[k] for the k-th scalar behind the cut (int32 device permutation)."""
    _check_data(solver, data, "schur_complement")
    _check_device(solver, "schur_complement", data)
    bar = _check_span(solver, span, "schur_complement")
    if bar == solver.order():
        raise ValueError("schur_complement: no span behind span %d" % span)
    _check_dest(solver, data, bar, dest, "schur_complement")
    return _SchurComplement.apply(solver, data, span, dest)


def solve_l_up_to(solver, P, span, b):
    """y = [L11 0; L21 I]^-1 b for a partial factor P from factor_up_to() (Solver.solveLUpTo),
    differentiable in P and b (b as for solve).  y[bar:] is the reduced right-hand side
    b2 - A21 A11^-1 b1."""
    _check_data(solver, P, "solve_l_up_to")
    _check_rhs(solver, P, b, "solve_l_up_to")
    _check_device(solver, "solve_l_up_to", P, b)
    bar = _check_span(solver, span, "solve_l_up_to")
    return _SolveLUpTo.apply(solver, P, span, bar, b)
