"""Differentiable sparse symmetric solves from coordinate entries, in the caller's order.

    from baspacho_amd import sparse as S
    pat = S.SymmetricPattern(rows, cols, n)        # once per pattern: solver + assembly map
    x = S.solve(pat, values, b)                    # x = A^-1 b
    ld = S.logdet(pat, values)                     # log det A
    x, ld = S.solve_logdet(pat, values, b)         # both, one factor
    data = S.assemble(pat, values)                 # the solver's layout, for baspacho_amd.autograd
    x = S.sample(pat, values, z, mu)               # x = mu + L^-T z: Cov(x) = A^-1
    pat = S.SymmetricPattern(rows, cols, n, keep=kept)     # kept scalars ordered last
    Sk, rk = S.marginalize(pat, values, b)         # marginal precision / information of the kept scalars

The matrix is given by entries (rows[k], cols[k], values[k]) in the caller's scalar order: A_ij = A_ji =
the sum of the values of the entries at (i, j), i >= j.  `values` is [nnz] or a
batch [B, nnz] of matrices of one pattern; `b` and `x` are in the caller's order, [n] or [n, k], with a
leading B when batched.  Gradients go to `values` and `b` (and to `z` and `mu` for sample).

Each function composes the assembly kernel (whose backward is its adjoint), baspacho_amd.autograd's
solve / logdet / solve_logdet and a permutation of the vectors.  Everything runs on
torch.cuda.current_stream() without host synchronisation, and the solver's own stream is restored
afterwards; the first call on a device uploads the assembly map and the permutation.  Double backward
is not supported.

marginalize eliminates every scalar outside `keep`: S = A22 - A21 A11^-1 A12 and
r = b2 - A21 A11^-1 b1 with block 2 the kept scalars, rows and columns in the order of `keep`.  inv(S) is
the `keep` block of inv(A): S and r are the precision and the information vector of the marginal.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import Settings, SparseStructure, create_solver
from . import autograd as _ag
from .autograd import _OnCurrentStream

__all__ = ["SymmetricPattern", "assemble", "solve", "logdet", "solve_logdet", "sample", "marginalize"]


def _host_i64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def _block_structure(num_params, p, q):
    """lower block CSR (diagonal included) of the block pairs (p[k], q[k]), p >= q"""
    key = np.unique(np.concatenate([p * num_params + q, np.arange(num_params, dtype=np.int64) * (num_params + 1)]))
    r, c = key // num_params, key % num_params
    ptrs = np.zeros(num_params + 1, dtype=np.int64)
    np.add.at(ptrs, r + 1, 1)
    return SparseStructure(np.cumsum(ptrs), c)


class SymmetricPattern:
    """A solver and its assembly map for the symmetric pattern of the entries (rows[k], cols[k]),
    0 <= rows, cols < n, in the caller's scalar order.  Scalars are grouped into params of
    `param_sizes` (default: all 1) in order; the param-level lower block structure is derived from the
    entries and handed to create_solver (fill and ordering as `settings` say).  triangle: "lower"
    (every entry has row >= col) or "full" (entries with row < col are skipped; the caller asserts the
    matrix is symmetric).  Invalid entries are refused by the assembly, which names the first one.
    keep: caller-order scalar indices (distinct, covering whole params) that marginalize() keeps; their
    params are ordered behind all others, from span `keep_span` on."""

    def __init__(self, rows, cols, n, param_sizes=None, settings=None, triangle="lower", keep=None):
        rows, cols = _host_i64(rows), _host_i64(cols)
        if len(rows) != len(cols):
            raise ValueError("SymmetricPattern: %d rows for %d cols" % (len(rows), len(cols)))
        n = int(n)
        ps = np.ones(n, dtype=np.int64) if param_sizes is None else _host_i64(param_sizes)
        if np.any(ps < 1) or int(ps.sum()) != n:
            raise ValueError("SymmetricPattern: param sizes must be >= 1 and sum to n = %d" % n)
        starts = np.concatenate([[0], np.cumsum(ps)])
        # the structure takes the well-formed lower entries; the assembly refuses the others by name
        ok = (rows >= 0) & (rows < n) & (cols >= 0) & (cols < n) & (rows >= cols)
        param_of = lambda i: np.searchsorted(starts, i, side="right") - 1
        ss = _block_structure(len(ps), param_of(rows[ok]), param_of(cols[ok]))
        self.n = n
        self.param_sizes = ps
        self.structure = ss
        keep_params = ()
        if keep is not None:
            keep = _host_i64(keep)
            if len(keep) == 0 or np.any(keep < 0) or np.any(keep >= n) or len(np.unique(keep)) != len(keep):
                raise ValueError("SymmetricPattern: keep must hold distinct scalar indices in [0, %d), at least one" % n)
            keep_params = np.unique(param_of(keep))
            if int(ps[keep_params].sum()) != len(keep):
                raise ValueError("SymmetricPattern: keep must cover whole params (it touches %d params of %d "
                                 "scalars with %d indices)" % (len(keep_params), int(ps[keep_params].sum()), len(keep)))
        self.solver = create_solver(settings or Settings(), ps, ss, elim_last_ids=[int(p) for p in keep_params])
        self.assembly = self.solver.assembly(rows, cols, triangle)
        self.nnz = len(rows)
        perm = self.solver.scalarPermutation()
        self._to_user = perm                 # internal -> user: x_user = x_int[perm]
        self._to_internal = np.argsort(perm)  # user -> internal: v_int = v_user[inv]
        self._dev = {}
        self.keep = keep
        self.keep_span = None
        if keep is not None:
            sol, sk = self.solver, self.solver.skel()
            spans = np.sort(sol.paramToSpan()[keep_params])
            self.keep_span = int(spans[0])
            if not np.array_equal(spans, np.arange(self.keep_span, sol.numSpans())) \
                    or int(sk["spanOffsetInLump"][self.keep_span]) != 0:
                raise RuntimeError("SymmetricPattern: the solver did not place the kept params behind a lump "
                                   "boundary (spans %s of %d)" % (spans.tolist(), sol.numSpans()))
            bar = int(sk["spanStart"][self.keep_span])
            self._keep_internal = perm[keep]  # internal scalar of keep[t]
            dest = np.empty(n - bar, dtype=np.int32)
            dest[self._keep_internal - bar] = np.arange(len(keep), dtype=np.int32)
            self._keep_dest = dest            # position in keep of the k-th scalar behind the cut

    @staticmethod
    def from_torch(A, param_sizes=None, settings=None, triangle="lower"):
        """(pattern, values) of a square torch sparse COO or CSR tensor, duplicates of an uncoalesced
        COO tensor kept as separate entries.  Gradients are promised only for the `values` tensor
        passed explicitly to the functions of this module."""
        if A.dim() != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("from_torch: expected a square matrix, got shape %s" % (tuple(A.shape),))
        if A.layout == torch.sparse_coo:
            idx, values = A._indices(), A._values()
            rows, cols = idx[0], idx[1]
        elif A.layout == torch.sparse_csr:
            crow = A.crow_indices()
            rows = torch.repeat_interleave(torch.arange(A.shape[0], device=crow.device), crow[1:] - crow[:-1])
            cols, values = A.col_indices(), A.values()
        else:
            raise TypeError("from_torch: expected a sparse COO or CSR tensor, got layout %s" % A.layout)
        pat = SymmetricPattern(rows, cols, A.shape[0], param_sizes, settings, triangle)
        return pat, values.detach()

    def _index(self, which, device):
        key = (which, device)
        if key not in self._dev:
            src = {"to_internal": self._to_internal, "to_user": self._to_user,
                   "keep_internal": getattr(self, "_keep_internal", None),
                   "keep_dest": getattr(self, "_keep_dest", None)}[which]
            self._dev[key] = torch.from_numpy(src).to(device)
        return self._dev[key]

    def _permute(self, v, which, dim, what):
        if not isinstance(v, torch.Tensor):
            raise TypeError("%s: expected a torch.Tensor, got %s" % (what, type(v).__name__))
        if v.dim() <= dim or v.shape[dim] != self.n:
            raise ValueError("%s: dimension %d of shape %s must be n = %d" % (what, dim, tuple(v.shape), self.n))
        return v.index_select(dim, self._index(which, v.device))

    def toInternal(self, v, dim=0):
        """v (dimension `dim` of size n) from the caller's order into the solver's internal order"""
        return self._permute(v, "to_internal", dim, "toInternal")

    def fromInternal(self, v, dim=0):
        """v from the solver's internal order back into the caller's order"""
        return self._permute(v, "to_user", dim, "fromInternal")


class _Assemble(torch.autograd.Function):
    @staticmethod
    def forward(ctx, asm, values):
        with _OnCurrentStream(asm.solver, values.device):
            data = asm.assemble(values.detach())
        ctx.asm = asm
        ctx.set_materialize_grads(False)
        return data

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None
        asm = ctx.asm
        with _OnCurrentStream(asm.solver, g.device):
            gv = asm.adjoint(g.contiguous())
        return None, gv


def _check_values(pattern, values, what):
    if not isinstance(pattern, SymmetricPattern):
        raise TypeError("%s: pattern must be a SymmetricPattern, got %s" % (what, type(pattern).__name__))
    if not isinstance(values, torch.Tensor):
        raise TypeError("%s: values must be a torch.Tensor, got %s" % (what, type(values).__name__))
    if values.dtype not in (torch.float64, torch.float32):
        raise TypeError("%s: values must be float64 or float32, got %s" % (what, values.dtype))
    if values.dim() not in (1, 2) or values.shape[-1] != pattern.nnz:
        raise ValueError("%s: values must be [%d] or [B, %d], got shape %s"
                         % (what, pattern.nnz, pattern.nnz, tuple(values.shape)))
    if values.dim() == 2 and values.shape[0] == 0:
        raise ValueError("%s: empty batch" % what)
    if not values.is_cuda:
        raise ValueError("%s: values must live in device memory, got a %s tensor" % (what, values.device))


def _check_b(pattern, values, b, what):
    if not isinstance(b, torch.Tensor):
        raise TypeError("%s: b must be a torch.Tensor, got %s" % (what, type(b).__name__))
    batched = values.dim() == 2
    lo = 2 if batched else 1
    if b.dim() not in (lo, lo + 1) or b.shape[lo - 1] != pattern.n:
        raise ValueError("%s: b must be %s with n = %d, got shape %s" % (
            what, "[B, n] or [B, n, k]" if batched else "[n] or [n, k]", pattern.n, tuple(b.shape)))
    if b.device != values.device:
        raise ValueError("%s: b is on %s, values on %s" % (what, b.device, values.device))
    return lo - 1


def assemble(pattern, values):
    """the solver's layout [dataSize] (or [B, dataSize]) of the entries' values, differentiable in
    values: its backward is the adjoint gather"""
    _check_values(pattern, values, "assemble")
    return _Assemble.apply(pattern.assembly, values)


def solve(pattern, values, b):
    """x = A(values)^-1 b in the caller's order, differentiable in values and b"""
    _check_values(pattern, values, "solve")
    dim = _check_b(pattern, values, b, "solve")
    x = _ag.solve(pattern.solver, assemble(pattern, values), pattern.toInternal(b, dim))
    return pattern.fromInternal(x, dim)


def logdet(pattern, values):
    """log det A(values): a 0-dim tensor, or [B] for a batch; differentiable in values"""
    _check_values(pattern, values, "logdet")
    return _ag.logdet(pattern.solver, assemble(pattern, values))


def solve_logdet(pattern, values, b):
    """(A(values)^-1 b, log det A(values)) from one factor, x in the caller's order"""
    _check_values(pattern, values, "solve_logdet")
    dim = _check_b(pattern, values, b, "solve_logdet")
    x, ld = _ag.solve_logdet(pattern.solver, assemble(pattern, values), pattern.toInternal(b, dim))
    return pattern.fromInternal(x, dim), ld


def sample(pattern, values, z, mu=None):
    """x = mu + P^T L^-T (P z) in the caller's order, P the solver's permutation and L the factor of
    A(values) in internal order, so that Cov(x) = A^-1 for z ~ N(0, I): a sample of the Gaussian with
    precision A.  z (and mu) are shaped like solve's b; differentiable in values, z and mu"""
    _check_values(pattern, values, "sample")
    dim = _check_b(pattern, values, z, "sample")
    if mu is not None:
        if not isinstance(mu, torch.Tensor) or mu.shape != z.shape:
            raise ValueError("sample: mu must be a tensor of z's shape %s" % (tuple(z.shape),))
    L = _ag.cholesky(pattern.solver, assemble(pattern, values))
    x = pattern.fromInternal(_ag.solve_lt(pattern.solver, L, pattern.toInternal(z, dim)), dim)
    return x if mu is None else mu + x


def marginalize(pattern, values, b=None):
    """S = A22 - A21 A11^-1 A12, [m, m] (or [B, m, m]), block 2 = pattern.keep, rows and columns in the order
    of keep: the marginal precision of the kept scalars.  With b ([n] or [n, k], leading B when batched)
    also r = b2 - A21 A11^-1 b1, [m] or [m, k]: their information vector.  Differentiable in values and b.
    Needs a pattern built with keep=..."""
    _check_values(pattern, values, "marginalize")
    if pattern.keep is None:
        raise ValueError("marginalize: the pattern was built without keep=...")
    sol, span = pattern.solver, pattern.keep_span
    dest = pattern._index("keep_dest", values.device)
    data = assemble(pattern, values)
    if b is None:
        return _ag.schur_complement(sol, data, span, dest=dest)
    dim = _check_b(pattern, values, b, "marginalize")
    if b.dtype != values.dtype:
        raise TypeError("marginalize: b has dtype %s, values have %s" % (b.dtype, values.dtype))
    P = _ag.factor_up_to(sol, data, span)
    S = _ag._SchurOfFactor.apply(sol, P, span, dest)
    y = _ag.solve_l_up_to(sol, P, span, pattern.toInternal(b, dim))
    return S, y.index_select(dim, pattern._index("keep_internal", values.device))
