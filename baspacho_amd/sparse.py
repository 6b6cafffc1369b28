"""Differentiable sparse symmetric solves from coordinate entries, in the caller's order.

    from baspacho_amd import sparse as S
    pat = S.SymmetricPattern(rows, cols, n)        # once per pattern: solver + assembly map
    x = S.solve(pat, values, b)                    # x = A^-1 b
    ld = S.logdet(pat, values)                     # log det A
    x, ld = S.solve_logdet(pat, values, b)         # both, one factor
    data = S.assemble(pat, values)                 # the solver's layout, for baspacho_amd.autograd
    x = S.sample(pat, values, z, mu)               # x = mu + L^-T z: Cov(x) = A^-1
    w = S.whiten(pat, values, x, mu)               # w = L^T (x - mu): |w|^2 = (x - mu)^T A (x - mu); undoes sample
    x = S.sample_cov(pat, values, z, mu)           # x = mu + L z: Cov(x) = A
    c = S.covariance(pat, values)                  # (A^-1)[rows[k], cols[k]] for every entry k
    v = S.marginal_variances(pat, values)          # diag(A^-1) in the caller's order
    c = S.cross_covariance(pat, values, i, j)      # (A^-1)[i[k], j[k]] for ANY scalar pairs, on or off the pattern
    C = S.joint_covariance(pat, values, idx)       # the dense [k, k] block of A^-1 on the scalars idx
    pat = S.SymmetricPattern(rows, cols, n, keep=kept)     # kept scalars ordered last
    Sk, rk = S.marginalize(pat, values, b)         # marginal precision / information of the kept scalars

    y = S.matvec(pat, values, x)                   # y = A x straight from the entries: the layout is never built
    q = S.quad_form(pat, values, x)                # x^T A x
    lp = S.log_prob(pat, values, x, mu)            # log N(x; mu, A^-1): the Gaussian whose precision is A
    x = S.solve_refined(pat, values, b, iters=3)   # fp32 factor + fp64 refinement on the entries' A x
    x, info = S.solve_refined(pat, values, b, iters=6, tol=1e-14, return_info=True)  # checked refinement
    e = S.backward_error(pat, values, x, b)        # max_i |b - A x|_i / (|A| |x| + |b|)_i per right-hand side
    k = S.cond_estimate(pat, values, scaled=True)  # kappa_1 of the Jacobi-scaled matrix, from the factor
    x = S.solve_cg(pat, values, b, precond="block_jacobi", tol=1e-10)  # device-resident PCG, no layout, no factor
    run = S.lanczos(pat, values, v0, steps=32)     # alpha, beta, stop words (and the basis) of Lanczos runs on A
    lo, hi = S.eig_extremes(pat, values, steps=64) # extreme eigenvalues by device-resident Lanczos, from the entries
    k2 = S.cond2_estimate(pat, values)             # kappa_2 = lam_max / lam_min (cond_estimate gives kappa_1)
    ld = S.logdet_slq(pat, values, probes=16)      # log det A without a factor: stochastic Lanczos quadrature
    y = S.apply_function(pat, values, v, "log")    # f(A) v without a factor: sqrt, inv_sqrt, inv, log, exp, pow, callable
    x = S.sample_lanczos(pat, values, z, mu)       # x = mu + A^{-1/2} z: Cov(x) = A^-1, the law of sample, no factor
    x = S.sample_cov_lanczos(pat, values, z, mu)   # x = mu + A^{1/2} z: Cov(x) = A

    jpat = S.JacobianPattern(jrows, jcols, m, n)   # once per Jacobian pattern: solver + normal-equations maps
    x = S.lstsq(jpat, jvalues, r, damping=(a, b))  # x = (J^T J + D)^-1 J^T r, D = a diag(J^T J) + b I
    st = S.check_positive_definite(pat, values)    # factor status: ok, or the caller's scalar of the first bad pivot
    data, g = S.normal_equations(jpat, jvalues, r) # H = J^T J in the layout and g = J^T r
    jop = S.JacobianOperator(jrows, jcols, m, n)   # the Jacobian as an operator: row and column lists, no layout
    x = S.lstsq_cg(jop, jvalues, r, damping=(a, b)) # the same step by CGLS from the entries: no pair list, no factor

The matrix is given by entries (rows[k], cols[k], values[k]) in the caller's scalar order: A_ij = A_ji =
the sum of the values of the entries at (i, j), i >= j.  `values` is [nnz] or a
batch [B, nnz] of matrices of one pattern; `b` and `x` are in the caller's order, [n] or [n, k], with a
leading B when batched.  Gradients go to `values` and `b` (and to `z` / `x` and `mu` for sample, whiten
and sample_cov, whose products with the factor are DESIGN.md section 22).

Each function composes the assembly kernel (whose backward is its adjoint), baspacho_amd.autograd's
solve / logdet / solve_logdet and a permutation of the vectors.  Everything runs on
torch.cuda.current_stream() without host synchronisation, and the solver's own stream is restored
afterwards; the first call on a device uploads the assembly map and the permutation.  Double backward
is not supported.

A JacobianPattern takes the entries (rows[k], cols[k], values[k]) of an m x n Jacobian, no position
repeated; H = J^T J is formed on the device straight in the solver's layout, in a
fixed summation order.  hessian / jt_vec / j_vec / normal_equations / lstsq are differentiable in the
Jacobian values and the vectors, and in the two damping factors when they are tensors.

lstsq_cg solves the same damped least-squares step matrix-free: CGLS on the row and
column lists of a JacobianOperator (or of JacobianPattern.operator), the residual r - J x kept in m-space, the
scalars of the iteration in solve_cg's state records; differentiable in the Jacobian values, r and the damping
factors.  j_vec and jt_vec take a JacobianOperator as well.

covariance and marginal_variances read A^-1 on the pattern from a selected inversion of the factor
(assemble -> cholesky -> selected_inverse -> a gather) and are differentiable in
values; their backward sweep adds with float atomics, so gradients are close, not bitwise, from run to
run.

cross_covariance and joint_covariance read entries of A^-1 anywhere, from forward solves over the reach of
the queried params alone (assemble -> factor -> Solver.inverseBlocks -> a gather), for
one matrix; they are differentiable in values, and their backward (columns of A^-1, then
Solver.patternGrad) is bitwise reproducible.

matvec, quad_form and log_prob multiply by A straight from the entries (DESIGN.md section 21:
SymmetricPattern.product, built on first use): no layout, no fill, a fixed summation order, gradients for
values and the vectors.  solve_refined factors the fp32 layout once and corrects the solution with fp64
residuals b - A x from the fp64 entries; the fp64 layout is never allocated, and its backward needs neither
patternGrad nor the assembly adjoint.

apply_function, sample_lanczos and sample_cov_lanczos apply a function of A to vectors from a Lanczos run on
the entries: f(A) v ~ |v| V f(T_k) e_1, the k x k part on the host and V y by one pass of
the combine kernel over the basis, or, with memory="two_pass", over a basis that a second run regenerates.
They are differentiable in the vectors and refuse values that require grad.

marginalize eliminates every scalar outside `keep`: S = A22 - A21 A11^-1 A12 and
r = b2 - A21 A11^-1 b1 with block 2 the kept scalars, rows and columns in the order of `keep`.  inv(S) is
the `keep` block of inv(A): S and r are the precision and the information vector of the marginal.
"""
import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import Settings, SparseStructure, create_solver, _call, _count, _ptr_arg, _ptr_of, _suffix
from . import autograd as _ag
from .autograd import _OnCurrentStream

__all__ = ["SymmetricPattern", "JacobianPattern", "JacobianSchur", "assemble", "solve", "logdet", "solve_logdet", "sample", "marginalize",
           "covariance", "marginal_variances", "cross_covariance", "joint_covariance",
           "hessian", "jt_vec", "j_vec", "normal_equations", "lstsq", "check_positive_definite",
           "matvec", "quad_form", "log_prob", "solve_refined", "whiten", "sample_cov",
           # error bounds: none of these is differentiable
           "residual", "backward_error", "norm1", "cond_estimate",
           # conjugate gradient from the entries
           "solve_cg",
           # matrix-free least squares from the entries of a Jacobian
           "JacobianOperator", "lstsq_cg",
           # Lanczos from the entries: only logdet_slq is differentiable
           "lanczos", "eig_extremes", "cond2_estimate", "logdet_slq",
           # f(A) v from the Lanczos basis: differentiable in the vectors, not in values
           "apply_function", "sample_lanczos", "sample_cov_lanczos"]


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


class _Pattern:
    """what SymmetricPattern and JacobianPattern share: the params, the solver with the kept params
    ordered last, and the permutations between the caller's order and the solver's"""

    def _init_params(self, n, param_sizes):
        name = type(self).__name__
        n = int(n)
        ps = np.ones(n, dtype=np.int64) if param_sizes is None else _host_i64(param_sizes)
        if np.any(ps < 1) or int(ps.sum()) != n:
            raise ValueError("%s: param sizes must be >= 1 and sum to n = %d" % (name, n))
        starts = np.concatenate([[0], np.cumsum(ps)])
        self.n = n
        self.param_sizes = ps
        return lambda i: np.searchsorted(starts, i, side="right") - 1

    def _init_solver(self, ss, settings, keep, param_of):
        name, n, ps = type(self).__name__, self.n, self.param_sizes
        self.structure = ss
        keep_params = ()
        if keep is not None:
            keep = _host_i64(keep)
            if len(keep) == 0 or np.any(keep < 0) or np.any(keep >= n) or len(np.unique(keep)) != len(keep):
                raise ValueError("%s: keep must hold distinct scalar indices in [0, %d), at least one" % (name, n))
            keep_params = np.unique(param_of(keep))
            if int(ps[keep_params].sum()) != len(keep):
                raise ValueError("%s: keep must cover whole params (it touches %d params of %d "
                                 "scalars with %d indices)" % (name, len(keep_params), int(ps[keep_params].sum()),
                                                               len(keep)))
        self.solver = create_solver(settings or Settings(), ps, ss, elim_last_ids=[int(p) for p in keep_params])
        self._keep_params = keep_params
        self._keep_arg = keep

    def _init_order(self):
        name, n, keep, keep_params = type(self).__name__, self.n, self._keep_arg, self._keep_params
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
                raise RuntimeError("%s: the solver did not place the kept params behind a lump "
                                   "boundary (spans %s of %d)" % (name, spans.tolist(), sol.numSpans()))
            bar = int(sk["spanStart"][self.keep_span])
            self._keep_internal = perm[keep]  # internal scalar of keep[t]
            dest = np.empty(n - bar, dtype=np.int32)
            dest[self._keep_internal - bar] = np.arange(len(keep), dtype=np.int32)
            self._keep_dest = dest            # position in keep of the k-th scalar behind the cut

    def _index(self, which, device):
        key = (which, device)
        if key not in self._dev:
            src = {"to_internal": self._to_internal, "to_user": self._to_user,
                   "diag": getattr(self, "_diag", None), "jrows": getattr(self, "_jrows", None),
                   "diag_user": getattr(self, "_diag_user", None),
                   "jcols": getattr(self, "_jcols", None),
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



class SymmetricPattern(_Pattern):
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
        param_of = self._init_params(n, param_sizes)
        n = self.n
        # the structure takes the well-formed lower entries; the assembly refuses the others by name
        ok = (rows >= 0) & (rows < n) & (cols >= 0) & (cols < n) & (rows >= cols)
        ss = _block_structure(len(self.param_sizes), param_of(rows[ok]), param_of(cols[ok]))
        self._init_solver(ss, settings, keep, param_of)
        self.assembly = self.solver.assembly(rows, cols, triangle)
        self.nnz = len(rows)
        self.triangle = triangle
        self._entries = (rows, cols)
        self._product = None
        self._init_order()
        # layout offset of the diagonal element of every scalar, in the caller's order
        self._diag_user = self.solver.diagOffsets()[self._to_user]

    @property
    def product(self):
        """the SymProduct of the entries, built on first use"""
        if self._product is None:
            self._product = self.solver.symProduct(self._entries[0], self._entries[1], self.triangle)
        return self._product

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


def _row_pairs(starts):
    """(a, b) positions with a >= b inside each group [starts[g], starts[g + 1]): every unordered pair
    of a group, self-pairs included, in ascending a"""
    d = np.diff(starts)
    total = int(starts[-1])
    pos = np.arange(total, dtype=np.int64) - np.repeat(starts[:-1], d)
    a = np.repeat(np.arange(total, dtype=np.int64), pos + 1)
    first = np.concatenate([[0], np.cumsum(pos + 1)])[:-1]
    b = np.arange(len(a), dtype=np.int64) - np.repeat(first, pos + 1) + np.repeat(np.arange(total) - pos, pos + 1)
    return a, b


class JacobianPattern(_Pattern):
    """A solver and the normal-equations maps for the m x n Jacobian with entries
    (rows[k], cols[k]), 0 <= rows < m, 0 <= cols < n, in the caller's scalar order, no position repeated.
    Scalars are grouped into params of `param_sizes` (default: all 1); two params are coupled in J^T J
    when one Jacobian row touches both, so the param-level lower block structure is the union of the
    rows' cliques, handed to create_solver (fill and ordering as `settings` say).  Invalid entries are
    refused by the map, which names the first one.  keep: as for SymmetricPattern."""

    def __init__(self, rows, cols, m, n, param_sizes=None, settings=None, keep=None):
        rows, cols = _host_i64(rows), _host_i64(cols)
        if len(rows) != len(cols):
            raise ValueError("JacobianPattern: %d rows for %d cols" % (len(rows), len(cols)))
        param_of = self._init_params(n, param_sizes)
        n, m = self.n, int(m)
        self.m = m
        # the structure takes the well-formed entries; the map refuses the others by name
        ok = (rows >= 0) & (rows < m) & (cols >= 0) & (cols < n)
        num_params = len(self.param_sizes)
        touch = np.unique(rows[ok] * num_params + param_of(cols[ok]))  # (row, param), sorted by row
        trow, tpar = touch // num_params, touch % num_params
        starts = np.concatenate([[0], np.cumsum(np.bincount(trow, minlength=max(m, 1)))]).astype(np.int64)
        a, b = _row_pairs(starts)
        ss = _block_structure(num_params, tpar[a], tpar[b])  # tpar ascends inside a row: tpar[a] >= tpar[b]
        self._init_solver(ss, settings, keep, param_of)
        self.normal_eq = self.solver.normalEquations(rows, cols, m)
        self.nnz = len(rows)
        self._init_order()
        self._diag = self.solver.diagOffsets()
        self._jrows, self._jcols = rows, cols
        self._operator = None

    @property
    def operator(self):
        """the JacobianOperator of the entries on this pattern's solver, built on first use"""
        if self._operator is None:
            self._operator = JacobianOperator._on(self.solver, self._jrows, self._jcols, self.m, self.n,
                                                  self.param_sizes)
        return self._operator


class JacobianOperator:
    """The m x n Jacobian with entries (rows[k], cols[k]) as an operator: the lists of its
    rows and columns for J v and J^T u, and the diagonal blocks of J^T J over the params, for lstsq_cg.  No
    layout, no pair list of the normal equations: the solver it holds is one over the block-diagonal structure
    of the params (default: all of size 1), whose analysis is trivial and whose layout is never allocated; it
    serves as the device context.  Invalid entries are refused by the map, which names the first one."""

    def __init__(self, rows, cols, m, n, param_sizes=None, settings=None):
        rows, cols = _host_i64(rows), _host_i64(cols)
        if len(rows) != len(cols):
            raise ValueError("JacobianOperator: %d rows for %d cols" % (len(rows), len(cols)))
        n = int(n)
        ps = np.ones(n, dtype=np.int64) if param_sizes is None else _host_i64(param_sizes)
        if np.any(ps < 1) or int(ps.sum()) != n:
            raise ValueError("JacobianOperator: param sizes must be >= 1 and sum to n = %d" % n)
        num = len(ps)
        ss = SparseStructure(np.arange(num + 1, dtype=np.int64), np.arange(num, dtype=np.int64))
        self._setup(create_solver(settings or Settings(), ps, ss), rows, cols, m, n, ps)

    @classmethod
    def _on(cls, solver, rows, cols, m, n, param_sizes):
        self = cls.__new__(cls)
        self._setup(solver, rows, cols, m, n, param_sizes)
        return self

    def _setup(self, solver, rows, cols, m, n, param_sizes):
        self.solver, self.m, self.n, self.nnz = solver, int(m), int(n), len(rows)
        self.param_sizes = param_sizes
        self.product = solver.jacobianProduct(rows, cols, self.m)
        self._jrows, self._jcols = rows, cols
        self._dev = {}
        self._schur = {}  # the maps of lstsq_cg(eliminate=indices), by the indices

    def _index(self, which, device):
        key = (which, device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy({"jrows": self._jrows, "jcols": self._jcols}[which]).to(device)
        return self._dev[key]


class JacobianSchur:
    """Implicit Schur elimination on a JacobianOperator: the params `eliminate` (indices into
    jop.param_sizes, any order; each at most 8 scalars, no Jacobian row touching two of them) are eliminated
    exactly and lstsq_cg(..., eliminate=this) runs the conjugate gradient on the reduced system of the kept ones.
    Holds the host map (Solver.jacobianSchur); build once, reuse across solves."""

    def __init__(self, jop, eliminate):
        if not isinstance(jop, JacobianOperator):
            raise TypeError("JacobianSchur: jop must be a JacobianOperator, got %s" % type(jop).__name__)
        self.jop = jop
        self.eliminate = _host_i64(eliminate)
        self.map = jop.solver.jacobianSchur(jop.product, eliminate)
        self.nK, self.nE = self.map.nK, self.map.nE
        self._kept = {}

    def info(self):
        return self.map.info()

    def table(self):
        return self.map.table()

    def kept_scalars(self, device):
        """int64 device tensor [nK]: the caller's scalar of every kept index"""
        if device not in self._kept:
            self._kept[device] = torch.from_numpy(self.map.table()["kept_scalar"].astype(np.int64)).to(device)
        return self._kept[device]


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


def _check_values(pattern, values, what, kind=SymmetricPattern):
    if not isinstance(pattern, kind):
        names = " or a ".join(k.__name__ for k in (kind if isinstance(kind, tuple) else (kind,)))
        raise TypeError("%s: pattern must be a %s, got %s" % (what, names, type(pattern).__name__))
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


def _check_mu(z, mu, what, name):
    if mu is not None:
        if not isinstance(mu, torch.Tensor) or mu.shape != z.shape:
            raise ValueError("%s: mu must be a tensor of %s's shape %s" % (what, name, tuple(z.shape)))


def whiten(pattern, values, x, mu=None):
    """w = P^T L^T P (x - mu) in the caller's order, P and L as for sample: the whitened residual of the
    Gaussian with precision A(values), so that w.square().sum(-1) (over the n scalars) is the quadratic
    form (x - mu)^T A (x - mu), and whiten(sample(z, mu), mu) = z.  x (and mu) are shaped like solve's b;
    differentiable in values, x and mu"""
    _check_values(pattern, values, "whiten")
    dim = _check_b(pattern, values, x, "whiten")
    _check_mu(x, mu, "whiten", "x")
    L = _ag.cholesky(pattern.solver, assemble(pattern, values))
    r = x if mu is None else x - mu
    return pattern.fromInternal(_ag.mul_lt(pattern.solver, L, pattern.toInternal(r, dim)), dim)


def sample_cov(pattern, values, z, mu=None):
    """x = mu + P^T L (P z) in the caller's order, P and L as for sample, so that Cov(x) = A for z ~ N(0, I):
    a sample of the Gaussian whose COVARIANCE is the sparse matrix.  z (and mu) are shaped like solve's b;
    differentiable in values, z and mu"""
    _check_values(pattern, values, "sample_cov")
    dim = _check_b(pattern, values, z, "sample_cov")
    _check_mu(z, mu, "sample_cov", "z")
    L = _ag.cholesky(pattern.solver, assemble(pattern, values))
    x = pattern.fromInternal(_ag.mul_l(pattern.solver, L, pattern.toInternal(z, dim)), dim)
    return x if mu is None else mu + x


class _GatherEntries(torch.autograd.Function):
    """the layout read at the entries (Assembly.adjoint: 0 for skipped entries); its backward is the
    assembly itself, which sums the gradients of the duplicates into their one slot"""

    @staticmethod
    def forward(ctx, asm, data):
        with _OnCurrentStream(asm.solver, data.device):
            out = asm.adjoint(data.detach().contiguous())
        ctx.asm = asm
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None
        asm = ctx.asm
        with _OnCurrentStream(asm.solver, g.device):
            gd = asm.assemble(g.contiguous())
        return None, gd


def _selected_inverse(pattern, values):
    sol = pattern.solver
    return _ag.selected_inverse(sol, _ag.cholesky(sol, assemble(pattern, values)))


def covariance(pattern, values):
    """c[k] = (A(values)^-1)[rows[k], cols[k]] for every entry k of the pattern, in the caller's order:
    [nnz], or [B, nnz] for a batch.  Duplicates all receive the value; entries the assembly skips (the
    upper half of a "full" pattern) get 0 and no gradient.  Differentiable in values."""
    _check_values(pattern, values, "covariance")
    return _GatherEntries.apply(pattern.assembly, _selected_inverse(pattern, values))


def marginal_variances(pattern, values):
    """diag(A(values)^-1) in the caller's order: [n], or [B, n] for a batch.  Differentiable in values."""
    _check_values(pattern, values, "marginal_variances")
    return _selected_inverse(pattern, values).index_select(-1, pattern._index("diag_user", values.device))


# ---- entries of A^-1 anywhere, by reach solves ------------------------------
_CROSS_BACKWARD_CHUNK = 256  # pairs per patternGrad call of the backward: U and V hold 2 x 256 x order values


class _CrossCovariance(torch.autograd.Function):
    """c[k] = (A(data)^-1)[rows[k], cols[k]], rows / cols internal scalars given as (param, offset) pairs.
    Backward: with x_i = A^-1 e_i, the data gradient of sum_k g_k e_i^T A^-1 e_j is patternGrad's formula
    with U = g_k x_{i_k}, V = x_{j_k}, alpha = -1."""

    @staticmethod
    def forward(ctx, solver, data, prm_i, off_i, prm_j, off_j, sizes):
        with _OnCurrentStream(solver, data.device):
            L = _ag._factor(solver, data)
            key = prm_i * len(sizes) + prm_j
            uniq, inv = np.unique(key, return_inverse=True)
            pairs = [(int(u // len(sizes)), int(u % len(sizes))) for u in uniq]
            offs = np.concatenate([[0], np.cumsum([sizes[p] * sizes[q] for p, q in pairs])]).astype(np.int64)
            flat = torch.empty(int(offs[-1]), dtype=data.dtype, device=data.device)
            if len(pairs):
                solver.inverseBlocks(L, pairs, out=flat)
            at = offs[inv] + off_i * sizes[prm_j] + off_j
            c = flat.index_select(0, torch.from_numpy(at).to(data.device))
        ctx.solver, ctx.q = solver, (prm_i, off_i, prm_j, off_j, sizes)
        ctx.save_for_backward(L)
        ctx.set_materialize_grads(False)
        return c

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        none = (None,) * 7
        if g is None or not ctx.needs_input_grad[1]:
            return none
        solver, (L,) = ctx.solver, ctx.saved_tensors
        prm_i, off_i, prm_j, off_j, sizes = ctx.q
        g = g.contiguous()
        total = None
        with _OnCurrentStream(solver, L.device):
            for k0 in range(0, len(prm_i), _CROSS_BACKWARD_CHUNK):
                k1 = min(k0 + _CROSS_BACKWARD_CHUNK, len(prm_i))
                prm = np.unique(np.concatenate([prm_i[k0:k1], prm_j[k0:k1]]))
                col0 = np.zeros(len(sizes), dtype=np.int64)
                col0[prm] = np.concatenate([[0], np.cumsum(sizes[prm])])[:-1]
                X = solver.inverseColumns(L, prm.tolist())  # [columns of prm, order], internal order
                ci = torch.from_numpy(col0[prm_i[k0:k1]] + off_i[k0:k1]).to(L.device)
                cj = torch.from_numpy(col0[prm_j[k0:k1]] + off_j[k0:k1]).to(L.device)
                U = (X.index_select(0, ci) * g[k0:k1, None]).contiguous()
                V = X.index_select(0, cj).contiguous()
                part = torch.empty_like(L)  # patternGrad writes and never adds
                solver.patternGrad(part, U=U, V=V, nRHS=k1 - k0, alpha=-1.0)
                total = part if total is None else total.add_(part)
        if total is None:
            total = torch.zeros_like(L)
        return (None, total) + (None,) * 5


def _scalar_queries(pattern, idx, what, name):
    """(param, offset inside the param) of caller-order scalar indices"""
    idx = _host_i64(idx)
    if np.any(idx < 0) or np.any(idx >= pattern.n):
        raise ValueError("%s: %s must hold scalar indices in [0, %d)" % (what, name, pattern.n))
    starts = np.concatenate([[0], np.cumsum(pattern.param_sizes)])
    prm = np.searchsorted(starts, idx, side="right") - 1
    return prm.astype(np.int64), (idx - starts[prm]).astype(np.int64)


def _check_single(pattern, values, what):
    _check_values(pattern, values, what)
    if values.dim() != 1:
        raise ValueError("%s: one matrix at a time: values must be [%d], got the batch shape %s"
                         % (what, pattern.nnz, tuple(values.shape)))
    _ag._check_device(pattern.solver, what, values)


def cross_covariance(pattern, values, rows, cols):
    """c[k] = (A(values)^-1)[rows[k], cols[k]] for any scalar pairs in the caller's order, on or off the
    pattern: [K].  rows / cols: host integer arrays (or tensors) of one length.  One matrix: a batch
    [B, nnz] is refused.  Differentiable in values."""
    what = "cross_covariance"
    _check_single(pattern, values, what)
    pi, oi = _scalar_queries(pattern, rows, what, "rows")
    pj, oj = _scalar_queries(pattern, cols, what, "cols")
    if len(pi) != len(pj):
        raise ValueError("%s: %d rows for %d cols" % (what, len(pi), len(pj)))
    return _CrossCovariance.apply(pattern.solver, assemble(pattern, values), pi, oi, pj, oj, pattern.param_sizes)


def joint_covariance(pattern, values, idx):
    """the dense symmetric block [k, k] of A(values)^-1 on the caller-order scalars idx (host integer array
    or tensor), symmetric to the last bit: the pairs a >= b by cross_covariance, mirrored.  One matrix: a
    batch [B, nnz] is refused.  Differentiable in values."""
    what = "joint_covariance"
    _check_single(pattern, values, what)
    idx = _host_i64(idx)
    _scalar_queries(pattern, idx, what, "idx")
    k = len(idx)
    a, b = np.tril_indices(k)
    c = cross_covariance(pattern, values, idx[a], idx[b])
    where = np.zeros((k, k), dtype=np.int64)
    where[a, b] = where[b, a] = np.arange(len(a))
    return c.index_select(0, torch.from_numpy(where.ravel()).to(values.device)).view(k, k)


def marginalize(pattern, values, b=None):
    """S = A22 - A21 A11^-1 A12, [m, m] (or [B, m, m]), block 2 = pattern.keep, rows and columns in the order
    of keep: the marginal precision of the kept scalars.  With b ([n] or [n, k], leading B when batched)
    also r = b2 - A21 A11^-1 b1, [m] or [m, k]: their information vector.  Differentiable in values and b.
    Needs a pattern built with keep=...  With a JacobianPattern, `values` are the Jacobian's and `b` is the
    residual r ([m] or [m, k]): A = J^T J and the right-hand side is J^T r."""
    jac = isinstance(pattern, JacobianPattern)
    _check_values(pattern, values, "marginalize", _Pattern)
    if pattern.keep is None:
        raise ValueError("marginalize: the pattern was built without keep=...")
    sol, span = pattern.solver, pattern.keep_span
    dest = pattern._index("keep_dest", values.device)
    data = hessian(pattern, values) if jac else assemble(pattern, values)
    if b is None:
        return _ag.schur_complement(sol, data, span, dest=dest)
    if jac:
        b = jt_vec(pattern, values, b)
    dim = _check_b(pattern, values, b, "marginalize")
    if b.dtype != values.dtype:
        raise TypeError("marginalize: b has dtype %s, values have %s" % (b.dtype, values.dtype))
    P = _ag.factor_up_to(sol, data, span)
    S = _ag._SchurOfFactor.apply(sol, P, span, dest)
    y = _ag.solve_l_up_to(sol, P, span, pattern.toInternal(b, dim))
    return S, y.index_select(dim, pattern._index("keep_internal", values.device))


# ---- normal equations of a sparse Jacobian ----------------------------------
class _Hessian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ne, values):
        v = values.detach().contiguous()
        with _OnCurrentStream(ne.solver, v.device):
            data = ne.hessian(v)
        ctx.ne = ne
        ctx.save_for_backward(v)
        ctx.set_materialize_grads(False)
        return data

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None
        ne, (v,) = ctx.ne, ctx.saved_tensors
        with _OnCurrentStream(ne.solver, g.device):
            gv = ne.hessianAdjoint(v, g.contiguous())
        return None, gv


def _products(jpat):
    """what runs J^T r and J v: the normal-equations maps of a JacobianPattern (one lane per run), the lists of
    a JacobianOperator (a wave for a long run); the same bits"""
    return jpat.product if isinstance(jpat, JacobianOperator) else jpat.normal_eq


_JACOBIANS = (JacobianPattern, JacobianOperator)


class _JVec(torch.autograd.Function):
    """transposed: J^T x (x [.., m(, q)]), else J x (x [.., n(, q)]).  The gradient of x is the other
    kernel on the incoming gradient; that of values[k] is the dot product over the q vectors of the two
    rows that entry k joins, an elementwise gather."""

    @staticmethod
    def forward(ctx, jpat, values, x, transposed):
        ne = _products(jpat)
        v, xc = values.detach().contiguous(), x.detach().contiguous()
        with _OnCurrentStream(ne.solver, v.device):
            out = ne.jtVec(v, xc) if transposed else ne.jVec(v, xc)
        ctx.jpat, ctx.transposed = jpat, transposed
        ctx.save_for_backward(v, xc)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        jpat, (v, x) = ctx.jpat, ctx.saved_tensors
        ne, g = _products(jpat), g.contiguous()
        gv = gx = None
        if ctx.needs_input_grad[2]:
            with _OnCurrentStream(ne.solver, g.device):
                gx = ne.jVec(v, g) if ctx.transposed else ne.jtVec(v, g)
        if ctx.needs_input_grad[1]:
            dim = v.dim() - 1
            rows, cols = jpat._index("jrows", g.device), jpat._index("jcols", g.device)
            of_rows, of_cols = (x, g) if ctx.transposed else (g, x)  # the [m]-sized and the [n]-sized side
            gv = of_rows.index_select(dim, rows) * of_cols.index_select(dim, cols)
            if gv.dim() > v.dim():
                gv = gv.sum(-1)
        return None, gv, gx, None


def _check_vec(jpat, values, x, size, what, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: %s must be a torch.Tensor, got %s" % (what, name, type(x).__name__))
    if x.dtype != values.dtype:
        raise TypeError("%s: %s has dtype %s, jvalues have %s" % (what, name, x.dtype, values.dtype))
    if x.device != values.device:
        raise ValueError("%s: %s is on %s, jvalues on %s" % (what, name, x.device, values.device))
    lo = values.dim()
    if x.dim() not in (lo, lo + 1) or x.shape[:lo - 1] != values.shape[:lo - 1] or x.shape[lo - 1] != size \
            or (x.dim() == lo + 1 and x.shape[-1] < 1):
        raise ValueError("%s: %s must be %s with %d rows, got shape %s" % (
            what, name, "[B, rows] or [B, rows, q]" if lo == 2 else "[rows] or [rows, q]", size, tuple(x.shape)))


def _damp(jpat, data, damping, what):
    """diag <- diag (1 + alpha) + beta, out of place over the unique diagonal offsets"""
    if damping is None:
        return data
    try:
        alpha, beta = damping
    except (TypeError, ValueError):
        raise TypeError("%s: damping must be a pair (alpha, beta), got %r" % (what, damping)) from None
    for name, t in (("alpha", alpha), ("beta", beta)):
        if isinstance(t, torch.Tensor):
            if t.dim() != 0:
                raise ValueError("%s: damping %s must be a float or a 0-dim tensor, got shape %s"
                                 % (what, name, tuple(t.shape)))
            if t.device != data.device:
                raise ValueError("%s: damping %s is on %s, jvalues on %s" % (what, name, t.device, data.device))
        elif not isinstance(t, (int, float)):
            raise TypeError("%s: damping %s must be a float or a 0-dim tensor, got %s" % (what, name, type(t).__name__))
    idx = jpat._index("diag", data.device)
    diag = data.index_select(-1, idx)
    return data.index_copy(-1, idx, (diag * (1 + alpha) + beta).to(data.dtype))


def hessian(jpat, jvalues, damping=None):
    """H = J^T J (+ D) in the solver's layout, [dataSize] or [B, dataSize], for baspacho_amd.autograd;
    damping = (alpha, beta): diag <- diag (1 + alpha) + beta, floats or 0-dim tensors.  Differentiable in
    jvalues, alpha and beta"""
    _check_values(jpat, jvalues, "hessian", JacobianPattern)
    return _damp(jpat, _Hessian.apply(jpat.normal_eq, jvalues), damping, "hessian")


def jt_vec(jpat, jvalues, r):
    """g = J^T r in the caller's order: r [m] or [m, q] -> [n] or [n, q] (leading B when batched).  jpat: a
    JacobianPattern, or a JacobianOperator, whose lists give a run of more than 64 entries to a whole wave"""
    _check_values(jpat, jvalues, "jt_vec", _JACOBIANS)
    _check_vec(jpat, jvalues, r, jpat.m, "jt_vec", "r")
    return _JVec.apply(jpat, jvalues, r, True)


def j_vec(jpat, jvalues, v):
    """y = J v: v [n] or [n, q] in the caller's order -> [m] or [m, q] (leading B when batched).  jpat as for
    jt_vec"""
    _check_values(jpat, jvalues, "j_vec", _JACOBIANS)
    _check_vec(jpat, jvalues, v, jpat.n, "j_vec", "v")
    return _JVec.apply(jpat, jvalues, v, False)


def normal_equations(jpat, jvalues, r, damping=None):
    """(data, g): H = J^T J (+ D) in the solver's layout and g = J^T r in the caller's order"""
    _check_values(jpat, jvalues, "normal_equations", JacobianPattern)
    _check_vec(jpat, jvalues, r, jpat.m, "normal_equations", "r")
    return _damp(jpat, _Hessian.apply(jpat.normal_eq, jvalues), damping, "normal_equations"), \
        _JVec.apply(jpat, jvalues, r, True)


def lstsq(jpat, jvalues, r, damping=None):
    """x = (J^T J + D)^-1 J^T r in the caller's order, [n] or [n, q]: the Gauss-Newton / Levenberg-Marquardt
    step of the residual r.  Differentiable in jvalues, r and the damping factors"""
    _check_values(jpat, jvalues, "lstsq", JacobianPattern)
    _check_vec(jpat, jvalues, r, jpat.m, "lstsq", "r")
    data, g = normal_equations(jpat, jvalues, r, damping)
    dim = jvalues.dim() - 1
    return jpat.fromInternal(_ag.solve(jpat.solver, data, jpat.toInternal(g, dim)), dim)


# ---- products with A straight from the entries ------------------------------
class _MatVec(torch.autograd.Function):
    """y = A(values) x from the entries.  A is symmetric: the gradient of x is A g, the same kernel on the
    incoming gradient; that of values[k] is g_r x_c + g_c x_r at the entry's (r, c) (g_r x_r on the
    diagonal), summed over the vectors: SymProduct.outer."""

    @staticmethod
    def forward(ctx, pattern, values, x):
        prod = pattern.product
        v, xc = values.detach().contiguous(), x.detach().contiguous()
        with _OnCurrentStream(prod.solver, v.device):
            out = prod.mv(v, xc)
        ctx.prod = prod
        ctx.save_for_backward(v, xc)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None
        prod, (v, x) = ctx.prod, ctx.saved_tensors
        g = g.contiguous()
        gv = gx = None
        with _OnCurrentStream(prod.solver, g.device):
            if ctx.needs_input_grad[1]:
                gv = prod.outer(g, x, batched=v.dim() == 2)
            if ctx.needs_input_grad[2]:
                gx = prod.mv(v, g)
        return None, gv, gx


def _check_x(pattern, values, x, what, name="x"):
    dim = _check_b(pattern, values, x, what)
    if x.dtype != values.dtype:
        raise TypeError("%s: %s has dtype %s, values have %s" % (what, name, x.dtype, values.dtype))
    if values.dim() == 2 and x.shape[0] != values.shape[0]:
        raise ValueError("%s: batch sizes differ: values hold %d matrices, %s holds %d"
                         % (what, values.shape[0], name, x.shape[0]))
    if x.dim() == dim + 2 and x.shape[-1] < 1:
        raise ValueError("%s: %s has no vectors" % (what, name))
    return dim


def matvec(pattern, values, x):
    """y = A(values) x in the caller's order, shaped like solve's b ([n] or [n, k], leading B when batched),
    straight from the entries: the layout is never assembled.  Differentiable in values and x."""
    _check_values(pattern, values, "matvec")
    _check_x(pattern, values, x, "matvec")
    return _MatVec.apply(pattern, values, x)


def quad_form(pattern, values, x):
    """sum_i x_i (A(values) x)_i: a 0-dim tensor for x [n], [k] for x [n, k], with a leading B when
    batched.  Differentiable in values and x."""
    _check_values(pattern, values, "quad_form")
    dim = _check_x(pattern, values, x, "quad_form")
    return (x * _MatVec.apply(pattern, values, x)).sum(dim)


def log_prob(pattern, values, x, mu=None):
    """log N(x; mu, A(values)^-1) = 0.5 logdet(pattern, values) - 0.5 quad_form(pattern, values, x - mu)
    - 0.5 n log(2 pi): the log-density of the Gaussian whose precision is A, mean mu (0 when None).  x (and mu)
    are shaped like solve's b; the result has the shape of quad_form.  Differentiable in values, x and mu."""
    _check_values(pattern, values, "log_prob")
    dim = _check_x(pattern, values, x, "log_prob")
    if mu is not None:
        if not isinstance(mu, torch.Tensor) or mu.shape != x.shape or mu.dtype != x.dtype:
            raise ValueError("log_prob: mu must be a tensor of x's shape %s and dtype %s" % (tuple(x.shape), x.dtype))
    d = x if mu is None else x - mu
    ld = logdet(pattern, values)
    qf = quad_form(pattern, values, d)
    if qf.dim() > ld.dim():
        ld = ld.unsqueeze(-1)
    return 0.5 * ld - 0.5 * qf - 0.5 * pattern.n * float(np.log(2.0 * np.pi))


def _berr(pattern, r, d, batched):
    """max_i |r_i| / d_i per column of residual's (r, d): [] / [k], with a leading B for a batch"""
    return pattern.solver.maxRatio(r, d, batched=batched)


def _refine(pattern, L32, v, b, iters, tol=None, want_info=False):
    """x = the fp32 solve of b through the factor L32, then `iters` corrections x += solve32(b - A x) with
    the residual in fp64 from the fp64 entries v; b and x in the caller's order, fp64.  With tol, a column
    whose backward error is <= tol before a correction keeps its x (a mask on the device).  want_info:
    (x, berr of x, corrections per column) from one more residual pass"""
    sol, prod = pattern.solver, pattern.product
    batched = v.dim() == 2
    dim = 1 if batched else 0
    has_k = b.dim() == dim + 2

    def solve32(r):
        rt = _ag._to_cols(pattern.toInternal(r.float(), dim), batched)
        _ag._solve_cols(sol, L32, rt)
        return pattern.fromInternal(_ag._from_cols(rt, r.shape), dim).double()

    b = b.contiguous()
    x = solve32(b)
    count = None
    if want_info:
        count = torch.zeros(b.shape[:dim] + (b.shape[-1:] if has_k else ()), dtype=torch.int64, device=b.device)
    for _ in range(iters):
        r, d = prod.residual(v, x.contiguous(), b)
        if tol is None:
            x = x + solve32(r)
            if want_info:
                count += 1
            continue
        active = _berr(pattern, r, d, batched) > tol
        x = torch.where(active.unsqueeze(-2 if has_k else -1), x + solve32(r), x)
        if want_info:
            count += active
    x = x.contiguous()
    if not want_info:
        return x
    r, d = prod.residual(v, x, b)
    return x, _berr(pattern, r, d, batched), count


class _SolveRefined(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, values, b, iters, tol=None, want_info=False):
        sol = pattern.solver
        v = values.detach().contiguous()
        with _OnCurrentStream(sol, v.device):
            L32 = pattern.assembly.assemble(v.float())
            members = _ag._members(L32) if L32.dim() == 2 else L32
            sol.factor(members)
            if want_info:
                status = sol.factorStatus(members)
                x, berr, count = _refine(pattern, L32, v, b.detach(), iters, tol, True)
            else:
                x = _refine(pattern, L32, v, b.detach(), iters, tol)
        ctx.pattern, ctx.iters = pattern, iters
        ctx.save_for_backward(L32, v, x)
        ctx.set_materialize_grads(False)
        if not want_info:
            return x
        ctx.mark_non_differentiable(berr, count, status)
        return x, berr, count, status

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        if g is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None, None, None, None
        pattern, (L32, v, x) = ctx.pattern, ctx.saved_tensors
        gv = None
        with _OnCurrentStream(pattern.solver, g.device):
            gb = _refine(pattern, L32, v, g.contiguous(), ctx.iters)  # A is symmetric: the same loop, the same factor
            if ctx.needs_input_grad[1]:
                gv = pattern.product.outer(gb, x, batched=v.dim() == 2).neg_()
        return None, gv, gb if ctx.needs_input_grad[2] else None, None, None, None


def solve_refined(pattern, values, b, iters=3, tol=None, return_info=False):
    """x = A(values)^-1 b in the caller's order from an fp32 factor and fp64 iterative refinement: values and
    b are float64 (any other dtype is a TypeError).  values.float() is assembled into an fp32 layout and
    factored once; x starts as the fp32 solve of b and is corrected `iters` times by x += solve32(b - A x),
    the residual in fp64 straight from the fp64 entries (SymProduct.residual: bitwise b - matvec).  Nothing
    is read back to the host; the fp64 layout is never allocated, so the factor takes half the memory of
    solve's.  Differentiable in values and b: b's gradient is the same loop (always `iters` passes) on the
    incoming gradient with the saved fp32 factor, and the gradient of values is -outer(gb, x) read at the
    entries.

    tol: `iters` becomes the largest number of corrections.  Before every correction the componentwise
    backward error max_i |b - A x|_i / (|A| |x| + |b|)_i of every column is taken on the device, and a column
    at or below tol keeps its x from then on: a mask on the update, still without a read-back (the queued
    work is the same; DESIGN.md section 23 says what that costs).

    return_info=True: (x, info) at the cost of one more residual pass; info holds device tensors: "berr",
    the backward error of the returned x per column ([] / [k], leading B for a batch); "corrections", int64
    of the same shape, how many corrections each column took; "factor_status", the record of the fp32 factor
    from Solver.factorStatus ([4] / [B, 4]; Solver.readFactorStatus decodes it).

    A factor that breaks down in fp32 (a matrix that is not positive definite once rounded to fp32, or too
    ill-conditioned for it) yields non-finite values, as solve does, and a refinement that stagnates returns
    its last iterate.  The library now detects both: info["factor_status"] decodes to ok = False for the
    first, info["berr"] stays above the tolerance (with corrections == iters) for the second; what to do
    about it (solve in fp64, regularise) is the caller's decision."""
    what = "solve_refined"
    _check_values(pattern, values, what)
    dim = _check_b(pattern, values, b, what)
    if values.dtype != torch.float64 or b.dtype != torch.float64:
        raise TypeError("%s: values and b must be float64, got %s and %s" % (what, values.dtype, b.dtype))
    if values.dim() == 2 and b.shape[0] != values.shape[0]:
        raise ValueError("%s: batch sizes differ: values hold %d matrices, b holds %d"
                         % (what, values.shape[0], b.shape[0]))
    if b.dim() == dim + 2 and b.shape[-1] < 1:
        raise ValueError("%s: b has no right-hand sides" % what)
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 0:
        raise ValueError("%s: iters must be an integer >= 0, got %r" % (what, iters))
    if tol is not None and (isinstance(tol, bool) or not isinstance(tol, (int, float)) or not tol >= 0):
        raise ValueError("%s: tol must be None or a number >= 0, got %r" % (what, tol))
    _ag._check_device(pattern.solver, what, values, b)
    if not return_info:
        return _SolveRefined.apply(pattern, values, b, iters, None if tol is None else float(tol), False)
    x, berr, count, status = _SolveRefined.apply(pattern, values, b, iters, None if tol is None else float(tol), True)
    return x, {"berr": berr, "corrections": count, "factor_status": status}


# ---- conjugate gradient from the entries ---------------------------------------
def _cg_run(pattern, v, b, precond, tol, max_steps, check_every, x0, cache):
    """the iteration of solve_cg on detached, contiguous operands: (x shaped like b, the CgRun).  `cache`
    keeps what the preconditioner built from v, for the backward pass"""
    from . import cg as _cg
    sol, prod = pattern.solver, pattern.product
    batched = v.dim() == 2
    dim = 1 if batched else 0
    has_k = b.dim() == dim + 2
    shape3 = tuple(b.shape) if has_k else tuple(b.shape) + (1,)
    b3 = b.contiguous().reshape(shape3)
    if x0 is None:
        x3, r3 = torch.zeros_like(b3), b3.clone()
    else:
        x3 = x0.detach().contiguous().reshape(shape3).clone()
        r3 = prod.residual(v, x3, b3)[0]  # bitwise b - A x0
    q = shape3[-1]
    mv_args = {}

    def apply_a(p, ap):
        if "a" not in mv_args:  # the operands never move: their pointers are taken once
            mv_args["a"] = [_ptr_arg(t.unbind(0) if batched else [t], batched) for t in (v, p, ap)]
        pv, pp, pa = mv_args["a"]
        _call(prod._lib, "bsp_sym_product_mv_", batched, _suffix(v), sol._h, prod._h, pv, pp, ctypes.c_int64(q), pa,
              *_count(v, batched))
        return ap

    pc = None
    if precond in ("jacobi", "block_jacobi", "fsai"):
        if precond not in cache:
            cache[precond] = _cg.Preconditioner(prod, precond, v)
        pc = cache[precond]
    elif precond == "factor32":
        if "L32" not in cache:
            L32 = pattern.assembly.assemble(v.float())
            sol.factor(_ag._members(L32) if batched else L32)
            cache["L32"] = L32
        L32 = cache["L32"]

        def pc(r):
            rr = r if has_k else r.reshape(b.shape)
            rt = _ag._to_cols(pattern.toInternal(rr.float(), dim), batched)
            _ag._solve_cols(sol, L32, rt)
            return pattern.fromInternal(_ag._from_cols(rt, rr.shape), dim).double().reshape(shape3)
    elif precond is not None:
        def pc(r):
            z = precond(r if has_k else r.reshape(b.shape))
            if not isinstance(z, torch.Tensor) or z.shape != b.shape:
                raise ValueError("solve_cg: the preconditioner must return a tensor of shape %s" % (tuple(b.shape),))
            return z.reshape(shape3)
    run = _cg.CgRun(sol, b3, x3, r3, apply_a, pc, tol, max_steps).run(check_every)
    return x3.reshape(b.shape), run


class _SolveCG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, values, b, precond, tol, max_steps, check_every, x0):
        v = values.detach().contiguous()
        cache = {}
        with _OnCurrentStream(pattern.solver, v.device):
            x, run = _cg_run(pattern, v, b.detach(), precond, tol, max_steps, check_every, x0, cache)
            has_k = b.dim() == v.dim() + 1
            info = [t if has_k else t.squeeze(-1) for t in (run.iterations(), run.stop(), run.relres())]
            info.append(run.state if has_k else run.state.squeeze(-2))
            built = cache.get(precond) if isinstance(precond, str) else None
            status = built.status if built is not None and hasattr(built, "status") else torch.empty(0, device=v.device)
        ctx.pattern, ctx.cache, ctx.settings = pattern, cache, (precond, tol, max_steps, check_every)
        ctx.save_for_backward(v, x)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*info, status)
        return (x, *info, status)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        if g is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return (None,) * 8
        pattern, (v, x) = ctx.pattern, ctx.saved_tensors
        precond, tol, max_steps, check_every = ctx.settings
        gv = None
        with _OnCurrentStream(pattern.solver, g.device):
            # A is symmetric: the same iteration, the same preconditioner, on the incoming gradient
            gb, _ = _cg_run(pattern, v, g.contiguous(), precond, tol, max_steps, check_every, None, ctx.cache)
            if ctx.needs_input_grad[1]:
                gv = pattern.product.outer(gb, x, batched=v.dim() == 2).neg_()
        return (None, gv, gb if ctx.needs_input_grad[2] else None) + (None,) * 5


def solve_cg(pattern, values, b, precond="block_jacobi", tol=1e-10, max_steps=100, check_every=8, x0=None,
             return_info=False):
    """x = A(values)^-1 b in the caller's order by preconditioned conjugate gradient, straight from the
    entries: A p is matvec's kernel, the layout is never allocated (except for "factor32"), and the scalars of
    the iteration (alpha, beta, the residual norms, the stop reason) live in a state record on the device that
    the kernels read.  values [nnz] / [B, nnz], b [n] / [n, k] with a leading B for a batch, float64 or
    float32: every (matrix, right-hand side) is a problem of its own and stops on its own, when
    |r|^2 <= tol^2 |b|^2 for the recurrence residual r (converged), after max_steps iterations, on a breakdown
    (p.Ap or r.z not > 0: A or the preconditioner is not positive definite), on a non-finite sum, or at once
    for a zero b (x = 0).  A stopped problem is frozen by the kernels.

    precond: None; "jacobi" (z_i = r_i / A_ii); "block_jacobi" (the inverses of the diagonal blocks of the
    pattern's params, at most 32 scalars each: a ValueError names a wider one); "fsai" (the factorised sparse
    approximate inverse z = G^T G r, G lower triangular on the pattern of A's lower triangle with at most 32
    scalars per row: for the ill-conditioned matrix that is not block-diagonally dominant), all three built and
    applied on the device; "factor32" (float64 only: the fp32 layout is assembled and factored once and z = the fp32 solve of
    r, as in solve_refined: the mixed-precision pattern, with an iteration instead of a fixed number of
    corrections); or a callable r -> z on tensors shaped like b that enqueues device work.

    Iterations are queued in chunks of check_every; after each chunk the host reads the stop words once and
    stops queuing when no problem runs.  check_every=None queues max_steps iterations without any read.  The
    result is bitwise the same for every check_every.  x0: the start, shaped like b (default 0).

    return_info=True: (x, info), info = device tensors "iterations", "stop" (0 running .. 5 zero right-hand
    side, baspacho_amd.cg.STOPS) and "relres" = sqrt(rr / bb) of the recurrence residual, shaped [] / [k] with a
    leading B for a batch, "state", the int64 records themselves ([.., 12]; baspacho_amd.cg.read_state decodes
    them), and for a built-in preconditioner "precond_status", int64 [2] / [B, 2] = {the
    caller's scalar of the lowest bad pivot of the preconditioner or -1, the number of bad blocks (for "fsai":
    of rows of G, which are then zero)}.

    Differentiable in values and b (x0 gets no gradient): b's gradient is solve_cg of the incoming gradient
    with the same settings and the same preconditioner, that of values is -outer(gb, x); both are as exact as
    the two solves.  Runs on the current torch stream; no stream capture."""
    from . import cg as _cg
    what = "solve_cg"
    _check_values(pattern, values, what)
    dim = _check_x(pattern, values, b, what, "b")
    _cg.check_settings(what, tol, max_steps, check_every)
    if x0 is not None:
        if not isinstance(x0, torch.Tensor) or x0.shape != b.shape or x0.dtype != b.dtype or x0.device != b.device:
            raise ValueError("%s: x0 must be a %s tensor of b's shape %s on %s" % (what, b.dtype, tuple(b.shape), b.device))
    if isinstance(precond, str):
        if precond not in ("jacobi", "block_jacobi", "fsai", "factor32"):
            raise ValueError("%s: precond must be None, 'jacobi', 'block_jacobi', 'fsai', 'factor32' or a callable, "
                             "got %r" % (what, precond))
        if precond == "factor32" and values.dtype != torch.float64:
            raise TypeError("%s: precond 'factor32' needs float64 values and b, got %s" % (what, values.dtype))
        if precond == "block_jacobi" and int(pattern.param_sizes.max(initial=0)) > _cg.MAX_BLOCK:
            p = int(np.argmax(pattern.param_sizes > _cg.MAX_BLOCK))
            raise ValueError("%s: param %d has %d scalars; 'block_jacobi' takes params of at most %d"
                             % (what, p, int(pattern.param_sizes[p]), _cg.MAX_BLOCK))
    elif precond is not None and not callable(precond):
        raise ValueError("%s: precond must be None, 'jacobi', 'block_jacobi', 'fsai', 'factor32' or a callable, got %r"
                         % (what, precond))
    _ag._check_device(pattern.solver, what, values, b)
    x, iters, stop, relres, state, status = _SolveCG.apply(pattern, values, b, precond, float(tol), max_steps,
                                                           check_every, x0)
    if not return_info:
        return x
    info = {"iterations": iters, "stop": stop, "relres": relres, "state": state}
    if precond in ("jacobi", "block_jacobi", "fsai"):
        info["precond_status"] = status
    return x, info


# ---- matrix-free least squares from the entries -----------------------------------
def _cgls_damping(what, damping):
    """(alpha, beta) as given, checked like lstsq's damping"""
    try:
        alpha, beta = damping
    except (TypeError, ValueError):
        raise TypeError("%s: damping must be a pair (alpha, beta), got %r" % (what, damping)) from None
    for name, t in (("alpha", alpha), ("beta", beta)):
        if isinstance(t, torch.Tensor):
            if t.dim() != 0:
                raise ValueError("%s: damping %s must be a float or a 0-dim tensor, got shape %s"
                                 % (what, name, tuple(t.shape)))
        elif isinstance(t, bool) or not isinstance(t, (int, float)):
            raise TypeError("%s: damping %s must be a float or a 0-dim tensor, got %s" % (what, name, type(t).__name__))
    return alpha, beta


def _cgls_run(jop, v, r, c, ab, precond, tol, max_steps, check_every, x0, cache):
    """the iteration of lstsq_cg on detached, contiguous operands: (x shaped like c or J^T r, the CglsRun).
    `cache` keeps what was built from v (the column norms, the damping vector, the preconditioner) for the
    backward pass"""
    from . import cgls as _cgls
    if r is None and c is None:
        raise ValueError("lstsq_cg: r and c cannot both be absent")
    prod = jop.product
    batched = v.dim() == 2
    dim = 1 if batched else 0
    like = r if r is not None else c
    has_k = like.dim() == dim + 2
    lead = tuple(v.shape[:-1])
    q = like.shape[-1] if has_k else 1
    r3 = None if r is None else r.contiguous().reshape(lead + (jop.m, q))
    c3 = None if c is None else c.contiguous().reshape(lead + (jop.n, q))
    shape = lead + (jop.n,) + ((q,) if has_k else ())
    if "colsq" not in cache and (ab is not None or precond == "jacobi"):
        cache["colsq"] = _cgls.column_norms(prod, v)
    if "d" not in cache:
        cache["d"] = None if ab is None else _cgls.damping_vector(prod, cache["colsq"], ab[0], ab[1], v)
    d = cache["d"]
    x3 = torch.zeros(lead + (jop.n, q), dtype=v.dtype, device=v.device) if x0 is None else \
        x0.detach().contiguous().reshape(lead + (jop.n, q)).clone()
    pc = None
    if precond in ("jacobi", "block_jacobi"):
        if precond not in cache:
            cache[precond] = _cgls.Preconditioner(prod, precond, v, cache.get("colsq"), d)
        pc = cache[precond]
    elif precond is not None:
        def pc(s):
            z = precond(s if has_k else s.reshape(shape))
            if not isinstance(z, torch.Tensor) or z.shape != shape:
                raise ValueError("lstsq_cg: the preconditioner must return a tensor of shape %s" % (shape,))
            return z.reshape(s.shape)
    run = _cgls.CglsRun(prod, v, r3, c3, d, x3, x0 is not None, pc, tol, max_steps).run(check_every)
    return x3.reshape(shape), run


class _SchurPrecond:
    """a built-in preconditioner of the reduced system on the kept scalars, applied by bsp_jac_schur_precond_apply_*
    inside a cg.CgRun (section 24's apply on the kept block table)"""

    def __init__(self, smap, kind, v, colsq, d):
        self.smap, self.kind = smap, smap._KINDS[kind]
        self.values, self.status = smap.precondBuild(kind, v, colsq, d)

    def cg_apply(self, run):
        sm = self.smap
        _call(sm._lib, "bsp_jac_schur_precond_apply_", run.batched, run.sfx, sm.solver._h, sm._h, ctypes.c_int32(self.kind),
              ctypes.c_int64(run.q), *run._args("schur_precond", self.values, run.r, run.z), *run._tail, *run._count)


class _SchurJacobiPrecond:
    """the block diagonal of S itself on the kept params ("schur_jacobi"), built once from the
    cached inverses of the eliminated blocks and applied by bsp_jac_schur_sjacobi_apply_* inside a cg.CgRun"""

    def __init__(self, smap, v, binv, d):
        self.smap, self.kind = smap, 2  # (the apply is the block apply, kind 2; cg.CgRun asks for the kind)
        self.values, self.status = smap.schurJacobiBuild(v, binv, d)

    def cg_apply(self, run):
        sm = self.smap
        _call(sm._lib, "bsp_jac_schur_sjacobi_apply_", run.batched, run.sfx, sm.solver._h, sm._h, ctypes.c_int64(run.q),
              *run._args("schur_jacobi", self.values, run.r, run.z), *run._tail, *run._count)


def _schur_run(sch, v, r, c, ab, precond, tol, max_steps, check_every, x0, cache):
    """the reduced iteration of lstsq_cg(eliminate=...) on detached, contiguous operands: (x shaped like c or J^T r,
    the CgRun on the kept scalars).  `cache` keeps what was built from v (the column norms, the damping vector, the
    inverses of the eliminated blocks with their status) for the backward pass"""
    from . import cg as _cg
    from . import cgls as _cgls
    if r is None and c is None:
        raise ValueError("lstsq_cg: r and c cannot both be absent")
    jop, smap = sch.jop, sch.map
    prod = jop.product
    batched = v.dim() == 2
    like = r if r is not None else c
    has_k = like.dim() == v.dim() + 1
    lead = tuple(v.shape[:-1])
    q = like.shape[-1] if has_k else 1
    r3 = None if r is None else r.contiguous().reshape(lead + (jop.m, q))
    c3 = None if c is None else c.contiguous().reshape(lead + (jop.n, q))
    shape = lead + (jop.n,) + ((q,) if has_k else ())
    kshape = lead + (sch.nK,) + ((q,) if has_k else ())
    if "colsq" not in cache and (ab is not None or precond == "jacobi"):
        cache["colsq"] = _cgls.column_norms(prod, v)
    if "d" not in cache:
        cache["d"] = None if ab is None else _cgls.damping_vector(prod, cache["colsq"], ab[0], ab[1], v)
    d = cache["d"]
    if "binv" not in cache:
        cache["binv"], cache["eliminate_status"] = smap.build(v, d)
    binv = cache["binv"]
    mem = lambda t: None if t is None else _ptr_arg(t.unbind(0) if batched else [t], batched)
    count = _count(v, batched)
    # g = J^T r + c in full space: the normal product of section 28 without x and d
    if r3 is None:
        g = c3
    else:
        g = torch.empty(lead + (jop.n, q), dtype=v.dtype, device=v.device)
        _call(prod._lib, "bsp_cgls_normal_", batched, _suffix(v), jop.solver._h, prod._h, mem(v), mem(r3), None, None,
              mem(c3), ctypes.c_int64(q), mem(g), None, *count)
    t = torch.empty(lead + (jop.m, q), dtype=v.dtype, device=v.device)
    bk = smap.reduce(v, binv, g, t=t)
    fixed = {"v": mem(v), "binv": mem(binv), "d": mem(d), "t": mem(t)}
    state = {}

    def apply_a(p, ap):
        if "ap" not in fixed:
            fixed["p"], fixed["ap"] = mem(p), mem(ap)
        _call(prod._lib, "bsp_jac_schur_mv_", batched, _suffix(v), jop.solver._h, smap._h, ctypes.c_int64(q), fixed["v"],
              fixed["binv"], fixed["d"], fixed["p"], fixed["t"], fixed["ap"], state.get("ptr"), *count)
        return ap

    if x0 is None:
        xk = torch.zeros_like(bk)
        rk = bk.clone()
    else:  # only the kept part of the start is read; r_k = b_k - S x_k0 by one product
        x03 = x0.detach().reshape(lead + (jop.n, q))
        xk = x03.index_select(len(lead), sch.kept_scalars(v.device)).contiguous()
        rk = bk - smap.mv(v, binv, xk, d=d, t=t)
    pc = None
    if precond in ("jacobi", "block_jacobi"):
        if precond not in cache:
            cache[precond] = _SchurPrecond(smap, precond, v, cache.get("colsq"), d)
        pc = cache[precond]
    elif precond == "schur_jacobi":
        if precond not in cache:
            cache[precond] = _SchurJacobiPrecond(smap, v, binv, d)
        pc = cache[precond]
    elif precond is not None:
        def pc(s):
            z = precond(s if has_k else s.reshape(kshape))
            if not isinstance(z, torch.Tensor) or z.shape != kshape:
                raise ValueError("lstsq_cg: the preconditioner must return a tensor of shape %s" % (kshape,))
            return z.reshape(s.shape)
    run = _cg.CgRun(jop.solver, bk, xk, rk, apply_a, pc, tol, max_steps)
    state["ptr"] = ctypes.c_void_p(_ptr_of(run.state))
    run.run(check_every)
    x3 = smap.backSubstitute(v, binv, g, xk, t=t)
    return x3.reshape(shape), run


class _LstsqCG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, jop, values, r, alpha, beta, precond, tol, max_steps, check_every, x0, schur):
        v = values.detach().contiguous()
        ab = None if alpha is None else (float(alpha), float(beta))
        cache = {}
        solve = _cgls_run if schur is None else _schur_run
        on = jop if schur is None else schur
        with _OnCurrentStream(jop.solver, v.device):
            x, run = solve(on, v, r.detach(), None, ab, precond, tol, max_steps, check_every, x0, cache)
            has_k = r.dim() == v.dim() + 1
            info = [t if has_k else t.squeeze(-1) for t in (run.iterations(), run.stop(), run.relres())]
            info.append(run.state if has_k else run.state.squeeze(-2))
            built = cache.get(precond) if isinstance(precond, str) else None
            status = built.status if built is not None else torch.empty(0, device=v.device)
            estatus = cache["eliminate_status"] if schur is not None else torch.empty(0, device=v.device)
        ctx.jop, ctx.cache, ctx.ab, ctx.solve, ctx.on = jop, cache, ab, solve, on
        ctx.ab_dtypes = tuple(t.dtype if isinstance(t, torch.Tensor) else None for t in (alpha, beta))
        ctx.settings = (precond, tol, max_steps, check_every)
        ctx.save_for_backward(v, r.detach().contiguous(), x)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*info, status, estatus)
        return (x, *info, status, estatus)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        need = ctx.needs_input_grad
        if g is None or not (need[1] or need[2] or need[3] or need[4]):
            return (None,) * 11
        jop, (v, r, x), ab = ctx.jop, ctx.saved_tensors, ctx.ab
        precond, tol, max_steps, check_every = ctx.settings
        prod = jop.product
        gv = gr = ga = gb = None
        with _OnCurrentStream(jop.solver, g.device):
            # N is symmetric: the same iteration with the right-hand side c = g alone
            # (with eliminate: one more reduced solve; the returned x solves the same N x = g, so the formulas hold)
            w, _ = ctx.solve(ctx.on, v, None, g.contiguous(), ab, precond, tol, max_steps, check_every, None, ctx.cache)
            jw = prod.jVec(v, w)
            if need[2]:
                gr = jw
            if need[1]:
                dim = v.dim() - 1
                rows, cols = jop._index("jrows", g.device), jop._index("jcols", g.device)
                res = r - prod.jVec(v, x)  # the residual of the result, by a product
                wc, xc = w.index_select(dim, cols), x.index_select(dim, cols)
                gv = wc * res.index_select(dim, rows) - jw.index_select(dim, rows) * xc
                wx = wc * xc
                if gv.dim() > v.dim():
                    gv, wx = gv.sum(-1), wx.sum(-1)
                if ab is not None:
                    gv = gv - 2.0 * ab[0] * v * wx
        if ab is not None and (need[3] or need[4]):
            wx = w * x
            if wx.dim() > v.dim():
                wx = wx.sum(-1)
            if need[3]:
                ga = -(ctx.cache["colsq"] * wx.double()).sum().to(ctx.ab_dtypes[0])
            if need[4]:
                gb = -wx.double().sum().to(ctx.ab_dtypes[1])
        return (None, gv, gr, ga, gb) + (None,) * 6


def lstsq_cg(jop, jvalues, r, damping=None, precond="block_jacobi", tol=1e-10, max_steps=100, check_every=8, x0=None,
             return_info=False, eliminate=None):
    """x = (J^T J + D)^-1 J^T r in the caller's order by CGLS, the conjugate gradient on the normal equations
    that keeps the residual r - J x in m-space, straight from the entries of J: the Gauss-Newton / Levenberg-
    Marquardt step of lstsq without a layout, a pair list or a factor.  jop: a JacobianOperator, or a
    JacobianPattern (its .operator is used).  jvalues [nnz] / [B, nnz], r [m] / [m, k] with a leading B for a
    batch, float64 or float32: every (matrix, right-hand side) is a problem of its own, with its state record on
    the device, and stops on its own as solve_cg's problems do, on s = J^T (r - J x) - D x: |s|^2 <= tol^2 |J^T
    r|^2 (converged), max_steps, a breakdown (the curvature |J p|^2 + p^T D p or s.z not > 0), a non-finite
    sum, or at once for J^T r = 0 (x = 0).

    damping=(alpha, beta), floats or 0-dim tensors: D = diag(alpha colsq_i + beta), colsq_i the squared norm of
    column i of J, lstsq's damping.  precond: None; "jacobi" (1 / (colsq_i + d_i)); "block_jacobi" (the inverses
    of the diagonal blocks of J^T J + D over the params, at most 32 scalars each: a ValueError names a wider
    one), both built and applied on the device; or a callable s -> z on tensors shaped like x.  The block build is one
    wave per param: where a param gathers very many Jacobian rows (a camera with thousands of observations) it
    dominates a short solve, and "jacobi" is then the cheaper choice (DESIGN.md section 28 has the figures).  check_every, x0
    and return_info as for solve_cg; info has "iterations", "stop", "relres", "state" and, for a built-in
    preconditioner, "precond_status".

    Differentiable in jvalues, r, alpha and beta (x0 gets no gradient): one more run with the incoming gradient
    as the right-hand side, the same preconditioner and settings, then products and elementwise gathers.  Runs
    on the current torch stream; no stream capture, no double backward.

    eliminate: None, a JacobianSchur of this operator, or an array of param indices (the map
    is then built once and kept on the operator).  Those params are eliminated exactly (each at most 8 scalars, no
    Jacobian row touching two of them) and the conjugate gradient runs on the reduced system S x_k = b_k of the
    kept scalars, S = C - F^T B^-1 F reached through products alone; the eliminated part of x comes from the
    back-substitution x_e = B^-1 (g_e - F x_k).  The stop test is then on the reduced system: |r_k|^2 <= tol^2
    |b_k|^2 for the recurrence residual of S x_k = b_k, and a zero b_k stops at once with x_k = 0 (x_e = B^-1 g_e is
    still returned).  Only the kept part of x0 is read.  precond then acts on the kept scalars: None; "jacobi" (1 /
    (colsq_c + d_c), the diagonal of C); "block_jacobi" (the inverses of the diagonal blocks of C = J_k^T J_k + D_k
    over the kept params, at most 32 scalars each); "schur_jacobi" (the inverses of the diagonal
    blocks of S itself over the kept params, at most 32 scalars each, built once per solve from the inverses of the
    eliminated blocks; only with eliminate), built and applied on the device; or a callable on tensors shaped
    [nK(, k)] (with the batch's leading B).  info gains "eliminate_status", int64 [2] / [B, 2] = {the caller's scalar of the lowest bad pivot of
    the eliminated blocks or -1, the number of bad blocks (their inverses are zero)}.  Gradients as above, by one
    more reduced solve."""
    from . import cg as _cg
    what = "lstsq_cg"
    if isinstance(jop, JacobianPattern):
        jop = jop.operator
    _check_values(jop, jvalues, what, _JACOBIANS)
    _check_vec(jop, jvalues, r, jop.m, what, "r")
    _cg.check_settings(what, tol, max_steps, check_every)
    alpha = beta = None
    if damping is not None:
        alpha, beta = _cgls_damping(what, damping)
    if x0 is not None:
        shape = tuple(jvalues.shape[:-1]) + (jop.n,) + tuple(r.shape[jvalues.dim():])
        if not isinstance(x0, torch.Tensor) or tuple(x0.shape) != shape or x0.dtype != r.dtype or x0.device != r.device:
            raise ValueError("%s: x0 must be a %s tensor of shape %s on %s" % (what, r.dtype, shape, r.device))
    if isinstance(precond, str):
        if precond == "schur_jacobi" and eliminate is None:
            raise ValueError("%s: precond 'schur_jacobi' is the block diagonal of the reduced system and needs eliminate"
                             % what)
        if precond not in ("jacobi", "block_jacobi", "schur_jacobi"):
            raise ValueError("%s: precond must be None, 'jacobi', 'block_jacobi' or a callable (with eliminate also "
                             "'schur_jacobi'), got %r" % (what, precond))
        if precond in ("block_jacobi", "schur_jacobi"):
            sizes = np.asarray(jop.param_sizes).copy()
            if eliminate is not None:  # (only the kept params carry a block of the reduced system's preconditioner)
                el = eliminate.eliminate if isinstance(eliminate, JacobianSchur) else _host_i64(eliminate)
                sizes[el[(el >= 0) & (el < len(sizes))]] = 0
            if int(np.max(sizes, initial=0)) > _cg.MAX_BLOCK:
                p = int(np.argmax(sizes > _cg.MAX_BLOCK))
                raise ValueError("%s: param %d has %d scalars; '%s' takes params of at most %d"
                                 % (what, p, int(sizes[p]), precond, _cg.MAX_BLOCK))
    elif precond is not None and not callable(precond):
        raise ValueError("%s: precond must be None, 'jacobi', 'block_jacobi' or a callable, got %r" % (what, precond))
    schur = None
    if eliminate is not None:
        if isinstance(eliminate, JacobianSchur):
            if eliminate.jop is not jop:
                raise ValueError("%s: eliminate was built on another operator" % what)
            schur = eliminate
        else:
            key = tuple(int(e) for e in _host_i64(eliminate))
            if key not in jop._schur:
                jop._schur[key] = JacobianSchur(jop, eliminate)
            schur = jop._schur[key]
    _ag._check_device(jop.solver, what, jvalues, r)
    x, iters, stop, relres, state, status, estatus = _LstsqCG.apply(jop, jvalues, r, alpha, beta, precond, float(tol),
                                                                     max_steps, check_every, x0, schur)
    if not return_info:
        return x
    info = {"iterations": iters, "stop": stop, "relres": relres, "state": state}
    if precond in ("jacobi", "block_jacobi", "schur_jacobi"):
        info["precond_status"] = status
    if schur is not None:
        info["eliminate_status"] = estatus
    return x, info


# ---- Lanczos from the entries ----------------------------------------------------
def _entries_operator(pattern, v, q):
    """apply_a(x, out) of a LanczosRun: out = A(v) x by the entries' product, the pointers of out taken once"""
    sol, prod = pattern.solver, pattern.product
    batched = v.dim() == 2
    pv = _ptr_arg(v.unbind(0) if batched else [v], batched)
    fixed = {}

    def apply_a(x, out):
        if "out" not in fixed:
            fixed["out"] = _ptr_arg(out.unbind(0) if batched else [out], batched)
        _call(prod._lib, "bsp_sym_product_mv_", batched, _suffix(v), sol._h, prod._h, pv,
              _ptr_arg(x.unbind(0) if batched else [x], batched), ctypes.c_int64(q), fixed["out"], *_count(v, batched))
        return out
    return apply_a


def _inverse_operator(pattern, v):
    """apply_a(x, out) with out = A(v)^-1 x: assembles and factors once, every application is a solve"""
    sol = pattern.solver
    batched = v.dim() == 2
    dim = 1 if batched else 0
    L = pattern.assembly.assemble(v)
    members = _ag._members(L) if batched else L
    sol.factor(members)
    status = sol.factorStatus(members)

    def apply_a(x, out):
        xt = _ag._to_cols(pattern.toInternal(x, dim), batched)
        _ag._solve_cols(sol, L, xt)
        out.copy_(pattern.fromInternal(_ag._from_cols(xt, x.shape), dim))
        return out
    return apply_a, status


def _lanczos_start(pattern, values, v0, what, name="v0"):
    """v0 ([n] / [n, q], or with values' leading B) as the contiguous [(B,) n, q] start of a run, and whether it
    had the q axis"""
    dim = _check_x(pattern, values, v0, what, name)
    has_q = v0.dim() == dim + 2
    v3 = v0.detach().contiguous()
    return (v3 if has_q else v3.unsqueeze(-1)).contiguous(), has_q


def _shared_start(values, z, n):
    """the host probes z [n, q] as a device start [(B,) n, q] of values' dtype: a batch shares them"""
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(device=values.device, dtype=values.dtype)
    if values.dim() == 2:
        zt = zt.unsqueeze(0).expand(values.shape[0], n, zt.shape[-1])
    return zt.contiguous()


def _lanczos_run(pattern, v, v3, apply_a, steps, reorth, check_every, keep_basis, breakdown=None):
    from . import lanczos as _lz
    return _lz.LanczosRun(pattern.solver, v3, apply_a, steps, reorth, keep_basis, breakdown).run(check_every)


def lanczos(pattern, values, v0, steps=32, reorth="full", check_every=None, keep_basis=False, breakdown=None):
    """`steps` steps of the Lanczos recurrence of A(values) from the start vector(s) v0, straight from the
    entries (A v is matvec's kernel; no layout, no factor), with the scalars of the recurrence in a state record
    on the device.  values [nnz] / [B, nnz]; v0 [n] / [n, q] with a leading B for a batch,
    any nonzero vectors (the run normalises them); every (matrix, start vector) is a run of its own and stops on
    its own: after `steps` steps (at most 512), on an invariant subspace (ww <= breakdown^2 (alpha^2 +
    beta_prev^2), breakdown 64 eps by default: the Krylov space is exhausted and the Ritz values are
    eigenvalues), on a non-finite sum, or at once for a zero v0.  A stopped run is frozen by the kernels.

    reorth "full" orthogonalises every new vector twice against all earlier ones (classical Gram-Schmidt on
    the device: the basis of `steps` vectors is kept); None runs the plain three-term recurrence on two
    vectors, whose Ritz values lose orthogonality and repeat once one has converged.  Steps are queued in
    chunks of check_every with one read of the stop words per chunk; None queues all steps and reads nothing.
    The result is bitwise the same for every check_every.

    Returns a dict of device tensors shaped [] / [q] with a leading B for a batch: "alpha" and "beta" float64
    [.., steps] (T_k = tridiag(beta_0 .. beta_{k-2}; alpha_0 .. alpha_{k-1}) for k = steps done; zero beyond),
    "steps", "stop" (baspacho_amd.lanczos.STOPS), "state" (int64 [.., 12]; baspacho_amd.lanczos.read_state),
    and, with reorth "full" or keep_basis, "basis" [.., steps, n(, q)] in the caller's order, v_j at index j.
    baspacho_amd.lanczos.ritz and quadrature post-process one run's coefficients on the host.  Not
    differentiable.  Runs on the current torch stream; no stream capture."""
    from . import lanczos as _lz
    what = "lanczos"
    _check_values(pattern, values, what)
    _lz.check_settings(what, steps, reorth, check_every, breakdown)
    v3, has_q = _lanczos_start(pattern, values, v0, what)
    _ag._check_device(pattern.solver, what, values, v0)
    v = values.detach().contiguous()
    with _OnCurrentStream(pattern.solver, v.device):
        run = _lanczos_run(pattern, v, v3, _entries_operator(pattern, v, v3.shape[-1]), steps, reorth, check_every,
                           keep_basis, breakdown)
        sq = (lambda t, d: t) if has_q else (lambda t, d: t.squeeze(d))
        out = {"alpha": sq(run.alpha(), -2), "beta": sq(run.beta(), -2), "steps": sq(run.steps_done(), -1),
               "stop": sq(run.stop(), -1), "state": sq(run.state, -2)}
        if run.kept:
            basis = run.basis.movedim(0, -3)  # [slots, (B,) n, q] -> [(B,) slots, n, q]
            out["basis"] = sq(basis, -1)
    return out


def _ritz_columns(run):
    """per (member, column) of a finished run: (theta, tau, bound, steps, stop), on the host (synchronises)"""
    from . import lanczos as _lz
    coef = run.coef.cpu().numpy().reshape(-1, 2, run.steps)
    state = run.state.cpu().numpy().reshape(-1, 12)
    out = []
    for c in range(coef.shape[0]):
        k, stop = int(state[c, 0]), int(state[c, 1])
        r = _lz.ritz(coef[c, 0], coef[c, 1], k) if k >= 1 and np.isfinite(coef[c, :, :k]).all() else None
        out.append((r, k, stop))
    return out


def eig_extremes(pattern, values, steps=64, v0=None, seed=0, method="entries", return_info=False):
    """(lam_min, lam_max): estimates of the extreme eigenvalues of A(values) from `steps` Lanczos steps with full
    reorthogonalisation, Python floats, or float64 numpy arrays [B] for a batch.  v0: the
    start vector [n] (a device tensor, shared by a batch); default: Rademacher signs from `seed`
    (baspacho_amd.lanczos.rademacher).  method "entries": both are the extreme Ritz values of one run on A, from
    the entries alone; Ritz values lie inside the spectrum, so lam_max is a lower and lam_min an upper bound,
    and lam_min converges slowly when the small eigenvalues are clustered relative to the spread.  method
    "factor": lam_min = 1 / theta_max of a second run on A^-1 (the layout is assembled and factored once, every
    step is a solve), where the smallest eigenvalue is the best separated one.  return_info=True: (lam_min,
    lam_max, info), info = {"bound_min", "bound_max": the residual bounds |beta_{k-1} s_{k-1,i}| of the two Ritz
    values (for "factor", bound_min is that of theta_max of A^-1), "steps", "stop": per run}.  A run that took no
    step or met a non-finite sum gives NaN.  Synchronises (the coefficients are read); not differentiable."""
    from . import lanczos as _lz
    what = "eig_extremes"
    _check_values(pattern, values, what)
    _lz.check_settings(what, steps, "full")
    if method not in ("entries", "factor"):
        raise ValueError("%s: method must be 'entries' or 'factor', got %r" % (what, method))
    n = pattern.n
    batched = values.dim() == 2
    if v0 is None:
        v3 = _shared_start(values, _lz.rademacher(n, 1, seed, values.dtype), n)
    else:
        if not isinstance(v0, torch.Tensor) or v0.shape != (n,):
            raise ValueError("%s: v0 must be a tensor of shape [%d], got %r" % (what, n, getattr(v0, "shape", v0)))
        if v0.dtype != values.dtype:
            raise TypeError("%s: v0 has dtype %s, values have %s" % (what, v0.dtype, values.dtype))
        v3 = v0.detach().reshape(n, 1)
        v3 = (v3.unsqueeze(0).expand(values.shape[0], n, 1) if batched else v3).contiguous()
    _ag._check_device(pattern.solver, what, values, v3)
    v = values.detach().contiguous()
    steps = min(steps, n)
    with _OnCurrentStream(pattern.solver, v.device):
        top = _ritz_columns(_lanczos_run(pattern, v, v3, _entries_operator(pattern, v, 1), steps, "full", None, False))
        low = top
        if method == "factor":
            low = _ritz_columns(_lanczos_run(pattern, v, v3, _inverse_operator(pattern, v)[0], steps, "full", None, False))
    nan = float("nan")
    lam_max = np.array([r[0][-1] if r is not None else nan for r, _, _ in top])
    bound_max = np.array([r[2][-1] if r is not None else nan for r, _, _ in top])
    if method == "factor":
        with np.errstate(all="ignore"):
            lam_min = np.array([1.0 / r[0][-1] if r is not None else nan for r, _, _ in low])
        bound_min = np.array([r[2][-1] if r is not None else nan for r, _, _ in low])
    else:
        lam_min = np.array([r[0][0] if r is not None else nan for r, _, _ in low])
        bound_min = np.array([r[2][0] if r is not None else nan for r, _, _ in low])
    pick = (lambda a: a) if batched else (lambda a: a[0].item())
    if not return_info:
        return pick(lam_min), pick(lam_max)
    # per matrix {the run on A, the run for lam_min (the same one for "entries")}
    counts = np.array([[k for _, k, _ in t] for t in (top, low)]).T
    stops = np.array([[s for _, _, s in t] for t in (top, low)]).T
    info = {"bound_min": pick(bound_min), "bound_max": pick(bound_max),
            "steps": counts if batched else counts[0].tolist(), "stop": stops if batched else stops[0].tolist()}
    return pick(lam_min), pick(lam_max), info


def cond2_estimate(pattern, values, steps=32, method="factor", return_info=False):
    """An estimate of the 2-norm condition number kappa_2(A) = lam_max / lam_min of A(values) from
    eig_extremes(pattern, values, steps, method=method): a Python float, or a float64 numpy array [B].  With
    method "entries" it is a lower bound of kappa_2, because Ritz values lie inside the spectrum (lam_max is
    under-, lam_min overestimated), and it never decreases with `steps`; with "factor" lam_min comes from A^-1
    and is underestimated instead, so the estimate may lie on either side of kappa_2, within the residual bounds
    that return_info reports (eig_extremes's info), and converges in a few dozen steps.  kappa_2 bounds the
    steps of solve_cg (about sqrt(kappa_2) log(2 / tol) / 2) and tells whether A is positive definite at all
    (lam_min <= 0).  cond_estimate gives kappa_1 instead, from a factor and Hager's 1-norm estimator; for a
    symmetric matrix kappa_1 / n <= kappa_2 <= n kappa_1, and kappa_1 is the number that bounds the error of a
    factor solve in the 1-norm.  Synchronises; not differentiable."""
    out = eig_extremes(pattern, values, steps=steps, method=method, return_info=return_info)
    with np.errstate(all="ignore"):
        kappa = out[1] / out[0]
    return (kappa, out[2]) if return_info else kappa


def _slq_forward(pattern, v, z3, steps, reorth):
    """(estimate per member [nb], terms [nb, q], steps, stops) of the quadrature of log on the probes z3"""
    from . import FactorizationError
    n, q = z3.shape[-2], z3.shape[-1]
    run = _lanczos_run(pattern, v, z3, _entries_operator(pattern, v, q), steps, reorth, None, False)
    cols = _ritz_columns(run)
    nb = len(cols) // q
    terms = np.zeros((nb, q))
    for i, (r, k, stop) in enumerate(cols):
        m, c = divmod(i, q)
        where = "probe %d" % c + (" of batch member %d" % m if v.dim() == 2 else "")
        if r is None:
            raise FactorizationError("logdet_slq: the run of %s took %d steps and stopped with '%s'"
                                     % (where, k, _stop_name(stop)), {"probe": c, "member": m, "stop": stop})
        theta, tau, _ = r
        if not theta[0] > 0:
            raise FactorizationError("logdet_slq: %s ends with the Ritz value %g <= 0: the matrix is not positive "
                                     "definite" % (where, theta[0]), {"probe": c, "member": m, "theta_min": float(theta[0])})
        terms[m, c] = n * float(np.sum(tau * np.log(theta)))
    state = run.state.cpu().numpy().reshape(nb, q, 12)
    return terms.mean(axis=1), terms, state[..., 0], state[..., 1]


def _stop_name(stop):
    from . import lanczos as _lz
    return _lz.STOPS[stop] if 0 <= stop < len(_lz.STOPS) else str(stop)


class _LogdetSLQ(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, values, z3, steps, reorth, cg):
        v = values.detach().contiguous()
        with _OnCurrentStream(pattern.solver, v.device):
            est, terms, k, stop = _slq_forward(pattern, v, z3, steps, reorth)
        dev = lambda a, dt: torch.from_numpy(np.array(a)).to(device=v.device, dtype=dt)  # (0-dim stays 0-dim)
        batched = v.dim() == 2
        pick = (lambda a: a) if batched else (lambda a: a[0])
        out = dev(pick(est), torch.float64)
        info = (dev(pick(terms), torch.float64), dev(pick(k), torch.int64), dev(pick(stop), torch.int64))
        ctx.pattern, ctx.cg = pattern, cg
        ctx.save_for_backward(v, z3)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*info)
        return (out, *info)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        if g is None or not ctx.needs_input_grad[1]:
            return (None,) * 6
        pattern, (v, z3) = ctx.pattern, ctx.saved_tensors
        n, q = z3.shape[-2], z3.shape[-1]
        kw = dict(precond="block_jacobi", tol=1e-10, max_steps=200, check_every=8)
        kw.update(ctx.cg or {})
        with _OnCurrentStream(pattern.solver, g.device):
            u, _ = _cg_run(pattern, v, z3, kw["precond"], float(kw["tol"]), kw["max_steps"], kw["check_every"], None, {})
            # A^-1 ~ (n / q) sum_c u_c z_c^T / (z_c . z_c): the gradient of the entries' values is its outer()
            scale = (float(n) / q) / (z3 * z3).sum(dim=-2, keepdim=True)
            gz = z3 * scale * g.to(v.dtype).reshape(g.shape + (1, 1))
            gv = pattern.product.outer(u.contiguous(), gz.contiguous(), batched=v.dim() == 2)
        return (None, gv) + (None,) * 4


def logdet_slq(pattern, values, probes=16, steps=32, seed=0, z=None, reorth="full", cg=None, return_info=False):
    """An estimate of log det A(values) without a factor, by stochastic Lanczos quadrature (DESIGN.md section
    25): (n / q) sum_c quadrature_c(log) over q probe vectors, where quadrature_c is the `steps`-point Gauss
    quadrature sum_i tau_i log(theta_i) of the Lanczos run started from probe c, run on the device straight from
    the entries.  A float64 device tensor [], or [B] for a batch [B, nnz], whose members share the probes.  The
    probes are `probes` Rademacher vectors from `seed` (baspacho_amd.lanczos.rademacher: the same seed gives the
    same probes), or the columns of z, a host array or tensor [n, q] of any nonzero vectors: the runs normalise
    their starts.  The identity as z gives the exact log det at steps = n (at O(n) runs: a test, not a method).
    The error of the estimate falls as 1 / sqrt(probes); its quadrature part falls geometrically in steps at a
    rate set by kappa_2 (cond2_estimate).  A probe whose run ends with a Ritz value <= 0 raises
    FactorizationError, which names the probe: the matrix is not positive definite.  Synchronises (the
    coefficients are read; the eigen-solves of the tridiagonals are host work).

    return_info=True: (estimate, info), info = {"terms": the per-probe values n quadrature_c(log), [q] / [B, q],
    whose mean is the estimate, "stderr": their standard error std(terms, ddof=1) / sqrt(q) (0 for one probe),
    "steps", "stop": per probe}.

    Differentiable in values.  The backward pass is the stochastic trace estimator on the same probes, not the
    derivative of the forward's floating-point value: with u_c = solve_cg(A, z_c) (cg = keyword arguments of
    solve_cg; default precond="block_jacobi", tol=1e-10, max_steps=200), grad_values = g (n / q) sum_c
    outer(u_c, z_c) / (z_c . z_c), the entries' share of (n / q) sum_c A^-1 z_c z_c^T / |z_c|^2.  It is an unbiased
    estimate of the true gradient, the entries' share of A^-1, for Rademacher probes, and exact (to the solves'
    tolerance) for identity probes.  Double backward is not supported; no stream capture."""
    from . import lanczos as _lz
    what = "logdet_slq"
    _check_values(pattern, values, what)
    _lz.check_settings(what, steps, reorth)
    n = pattern.n
    if z is None:
        if isinstance(probes, bool) or not isinstance(probes, int) or probes < 1:
            raise ValueError("%s: probes must be an integer >= 1, got %r" % (what, probes))
        zh = _lz.rademacher(n, probes, seed, np.float64)
    else:
        zh = z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else np.asarray(z)
        if zh.ndim != 2 or zh.shape[0] != n or zh.shape[1] < 1:
            raise ValueError("%s: z must be [%d, q] with q >= 1, got shape %s" % (what, n, tuple(zh.shape)))
        if zh.dtype.kind != "f":
            raise TypeError("%s: z must be a floating-point array, got %s" % (what, zh.dtype))
    if cg is not None and not isinstance(cg, dict):
        raise ValueError("%s: cg must be None or a dict of solve_cg's keyword arguments, got %r" % (what, cg))
    if cg is not None and set(cg) - {"precond", "tol", "max_steps", "check_every"}:
        raise ValueError("%s: cg takes precond, tol, max_steps and check_every, got %s" % (what, sorted(cg)))
    _ag._check_device(pattern.solver, what, values)
    z3 = _shared_start(values, zh, n)
    est, terms, k, stop = _LogdetSLQ.apply(pattern, values, z3, min(steps, n), reorth, cg)
    if not return_info:
        return est
    q = z3.shape[-1]
    stderr = terms.std(dim=-1, unbiased=True) / float(np.sqrt(q)) if q > 1 else torch.zeros_like(est)
    return est, {"terms": terms, "stderr": stderr, "steps": k, "stop": stop}


# ---- f(A) v from the Lanczos basis ----------------------------------------------
def _matfun_run(pattern, v, x3, fs, settings):
    """(out [nf, (B,) n, q], info) of baspacho_amd.lanczos.apply_function on the entries' product"""
    from . import lanczos as _lz
    steps, reorth, memory, check_every, breakdown = settings
    return _lz.apply_function(pattern.solver, x3, _entries_operator(pattern, v, x3.shape[-1]), fs, steps, reorth,
                              memory, check_every, breakdown)


class _ApplyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, values, x3, fs, settings, box):
        v = values.detach().contiguous()
        with _OnCurrentStream(pattern.solver, v.device):
            out, box["info"] = _matfun_run(pattern, v, x3.detach().contiguous(), fs, settings)
        ctx.pattern, ctx.fs, ctx.settings = pattern, fs, settings
        ctx.save_for_backward(v)
        ctx.set_materialize_grads(False)
        return tuple(out.unbind(0))

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        if not ctx.needs_input_grad[2] or all(g is None for g in gs):
            return (None,) * 6
        pattern, (v,) = ctx.pattern, ctx.saved_tensors
        total = None
        with _OnCurrentStream(pattern.solver, v.device):
            for f, g in zip(ctx.fs, gs):
                if g is not None:  # f(A) is symmetric: the same call, the same settings, on the incoming gradient
                    gx = _matfun_run(pattern, v, g.contiguous(), [f], ctx.settings)[0][0]
                    total = gx if total is None else total + gx
        return (None, None, total, None, None, None)


def _is_function(f):
    return callable(f) or isinstance(f, str) or (isinstance(f, tuple) and len(f) == 2 and f[0] in ("exp", "pow")
                                                   and isinstance(f[1], (int, float)))


def apply_function(pattern, values, v, f, steps=64, reorth="full", memory="basis", check_every=None, breakdown=None,
                   return_info=False):
    """f(A(values)) v in the caller's order without a factor: the Lanczos approximation |v| V f(T_k) e_1 from k <=
    `steps` steps of the recurrence started from v, run on the device straight from the entries (A v is matvec's
    kernel, as in lanczos), with the k x k eigen-solve on the host and the tall-skinny product V y as one pass of
    the combine kernel over the basis.  values [nnz] / [B, nnz]; v [n] / [n, q], or for a
    batch [B, n, q], or [n] / [n, q] shared by the members; every (matrix, column) is a run of its own.  f: "sqrt",
    "inv_sqrt", "inv", "log", ("exp", t) for exp(-t A), ("pow", p) for A^p, or a callable on the float64 array of
    Ritz values; or a sequence of up to 4 of these, which returns a tuple, all from one pass over the basis and
    each bitwise the single-function call.  steps is capped at min(n, 512).

    The approximation converges geometrically in steps at a rate set by kappa_2 (cond2_estimate tells it: on a
    matrix with kappa_2 = 1e3 and n = 40, inv_sqrt is still 1e-2 off after 32 steps and exact to rounding at 40);
    steps = n with reorth "full" reproduces f(A) v to rounding.  memory "basis" keeps the k basis vectors
    (k n q values); "two_pass" (reorth None only, else ValueError) runs the recurrence twice, which is bitwise
    reproducible, and adds y_j v_j as v_j is regenerated: no basis, twice the products, and bitwise the result
    of "basis" with reorth None.  A zero column gives exactly +0; a column whose run met a non-finite sum gives
    NaN.  A Ritz value outside the domain of f (<= 0 for inv_sqrt, inv, log and non-integer pow, < 0 for sqrt)
    raises FactorizationError, which names the column: the matrix is not positive definite.

    return_info=True: (result, info), info = device tensors per column ([] / [q], leading B for a batch) "steps",
    "stop" (baspacho_amd.lanczos.STOPS), "theta_min", "theta_max" (the extreme Ritz values of the run) and
    "change" (a leading axis over the functions when f is a sequence) = |y_k - pad(y_{k-1})| / |y_k|, the relative
    difference between the last two approximations.  It is an indicator of convergence, not a bound: it ran 1.5
    to 8 times below the true error of inv_sqrt on the test matrix.

    Differentiable in v: f(A) is symmetric, so the gradient is the same call on the incoming gradient with the
    same settings.  Gradients in values (the Frechet derivative of f) are not provided: values that require
    grad raise ValueError.  Synchronises (the coefficients are read); double backward and stream capture are not
    supported."""
    from . import lanczos as _lz
    what = "apply_function"
    if isinstance(values, torch.Tensor) and values.requires_grad and torch.is_grad_enabled():
        raise ValueError("%s: gradients in values (the Frechet derivative of f) are not provided; pass "
                         "values.detach()" % what)
    _check_values(pattern, values, what)
    many = not _is_function(f)
    fs = list(f) if many and isinstance(f, (list, tuple)) else [f]
    if not 1 <= len(fs) <= _lz.MAX_FUNCTIONS:
        raise ValueError("%s: f must be one function or a sequence of 1 .. %d, got %d" % (what, _lz.MAX_FUNCTIONS, len(fs)))
    for g in fs:
        _lz.check_function(what, g)
    batched = values.dim() == 2
    if not isinstance(v, torch.Tensor):
        raise TypeError("%s: v must be a torch.Tensor, got %s" % (what, type(v).__name__))
    if batched and v.dim() in (1, 2) and v.shape[0] == pattern.n:   # shared by the members
        v = v.unsqueeze(0).expand((values.shape[0],) + tuple(v.shape))
    elif batched and v.dim() != 3:
        raise ValueError("%s: with values [B, nnz], v must be [B, n, q] or a shared [n] / [n, q] with n = %d, got shape %s"
                         % (what, pattern.n, tuple(v.shape)))
    dim = _check_x(pattern, values, v, what, "v")
    has_q = v.dim() == dim + 2
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError("%s: steps must be an integer >= 1, got %r" % (what, steps))
    steps = max(1, min(steps, pattern.n, _lz.MAX_STEPS))
    _lz.check_settings(what, steps, reorth, check_every, breakdown)
    if memory not in ("basis", "two_pass"):
        raise ValueError("%s: memory must be 'basis' or 'two_pass', got %r" % (what, memory))
    if memory == "two_pass" and reorth is not None:
        raise ValueError("%s: memory 'two_pass' regenerates the basis from the three-term recurrence and needs "
                         "reorth=None, got reorth=%r" % (what, reorth))
    _ag._check_device(pattern.solver, what, values, v)
    box = {}
    x3 = v if has_q else v.unsqueeze(-1)
    outs = _ApplyFunction.apply(pattern, values, x3, tuple(fs), (steps, reorth, memory, check_every, breakdown), box)
    outs = tuple(o if has_q else o.squeeze(-1) for o in outs)
    res = outs if many else outs[0]
    if not return_info:
        return res
    info = {}
    for k, a in box["info"].items():
        t = torch.from_numpy(np.ascontiguousarray(a)).to(values.device)
        t = t if has_q else t.squeeze(-1)
        info[k] = t[0] if k == "change" and not many else t
    return res, info


def _with_mean(x, mu, what):
    if mu is None:
        return x
    if not isinstance(mu, torch.Tensor) or mu.shape != x.shape:
        raise ValueError("%s: mu must be a tensor of the result's shape %s" % (what, tuple(x.shape)))
    return mu + x


def sample_lanczos(pattern, values, z, mu=None, **kw):
    """x = mu + A(values)^{-1/2} z without a factor, by apply_function(pattern, values, z, "inv_sqrt", **kw): Cov(x)
    = A^-1 for z ~ N(0, I), the law of sample, though not the same map as its L^-T z (A^{-1/2} is the symmetric
    square root).  For the GMRF precision whose fill makes the factor unaffordable; where the factor fits, sample
    is faster and exact.  The accuracy is apply_function's: geometric in steps at a rate set by kappa_2
    (cond2_estimate).  Differentiable in z and mu, not in values."""
    out = apply_function(pattern, values, z, "inv_sqrt", **kw)
    if kw.get("return_info"):
        return _with_mean(out[0], mu, "sample_lanczos"), out[1]
    return _with_mean(out, mu, "sample_lanczos")


def sample_cov_lanczos(pattern, values, z, mu=None, **kw):
    """x = mu + A(values)^{1/2} z without a factor, by apply_function(pattern, values, z, "sqrt", **kw): Cov(x) = A
    for z ~ N(0, I), the law of sample_cov.  Differentiable in z and mu, not in values."""
    out = apply_function(pattern, values, z, "sqrt", **kw)
    if kw.get("return_info"):
        return _with_mean(out[0], mu, "sample_cov_lanczos"), out[1]
    return _with_mean(out, mu, "sample_cov_lanczos")


# ---- error bounds; none of these is differentiable ---------------------------
def _detached(pattern, values, what):
    _check_values(pattern, values, what)
    return values.detach().contiguous()


def residual(pattern, values, x, b):
    """(r, d) of x as a solution of A(values) x = b, in the caller's order and shaped like b: r = b - A x,
    bitwise b - matvec(pattern, values, x), and d = |A| |x| + |b| with duplicates as separate terms, both from
    one pass over the entries (SymProduct.residual).  Not differentiable."""
    what = "residual"
    v = _detached(pattern, values, what)
    _check_x(pattern, values, x, what)
    _check_x(pattern, values, b, what, "b")
    if b.shape != x.shape:
        raise ValueError("%s: b has shape %s, x has %s" % (what, tuple(b.shape), tuple(x.shape)))
    with _OnCurrentStream(pattern.solver, v.device):
        return pattern.product.residual(v, x.detach().contiguous(), b.detach().contiguous())


def backward_error(pattern, values, x, b):
    """the componentwise backward error of x as a solution of A(values) x = b, max_i |b - A x|_i / (|A| |x| +
    |b|)_i per right-hand side: a float64 device tensor [] for b [n], [k] for [n, k], with a leading B for a
    batch.  It is the smallest eps for which (A + dA) x = b + db with |dA| <= eps |A| and |db| <= eps |b|
    (Oettli-Prager); 0 / 0 counts as 0, a non-zero residual over a zero denominator as +inf, and a NaN
    anywhere in the column gives NaN.  Not differentiable."""
    r, d = residual(pattern, values, x, b)
    with _OnCurrentStream(pattern.solver, r.device):
        return _berr(pattern, r, d, values.dim() == 2)


def _jacobi_scale(pattern, data):
    """s = 1 / sqrt(diag A) in the caller's order from the assembled layout `data` ([dataSize] or [B, ..])"""
    return 1.0 / torch.sqrt(data.index_select(-1, pattern._index("diag_user", data.device)))


def _norm1(pattern, v, s):
    """max_i (|A| 1)_i, or max_i s_i (|A| s)_i with the scale s ([n] / [B, n], caller's order)"""
    sol, prod = pattern.solver, pattern.product
    batched = v.dim() == 2
    if s is None:
        w = prod.absMv(v, torch.ones(v.shape[:-1] + (pattern.n,), dtype=v.dtype, device=v.device))
    else:
        w = s * prod.absMv(v, s.contiguous())
    return sol.colMax(w, batched=batched)


def norm1(pattern, values, scaled=False):
    """||A(values)||_1 = max_i (|A| 1)_i from the entries (duplicates as separate terms: an upper bound of the
    norm where duplicates cancel), a float64 device tensor [] or [B].  scaled=True: max_i s_i (|A| s)_i with
    s = 1 / sqrt(diag A), the 1-norm of the Jacobi-scaled matrix S A S; the matrix itself is never scaled
    (the diagonal is read from the assembled layout).  Not differentiable."""
    v = _detached(pattern, values, "norm1")
    with _OnCurrentStream(pattern.solver, v.device):
        s = _jacobi_scale(pattern, pattern.assembly.assemble(v)) if scaled else None
        return _norm1(pattern, v, s)


def cond_estimate(pattern, values, scaled=False, return_info=False):
    """An estimate of the 1-norm condition number kappa_1(A) = ||A||_1 ||A^-1||_1 of A(values): assembles,
    factors, and returns norm1 * Solver.invNorm1 as a float64 device tensor [] or [B] (a lower bound, almost
    always within a factor 3 of the truth).  scaled=True estimates kappa_1(S A S), S = diag(A)^-1/2: the
    number that bounds the error of a Cholesky solve (van der Sluis), where the raw kappa_1(A) of a badly
    scaled matrix says nothing.  return_info=True: (estimate, info), info = {"state": the estimator's
    state record (Solver.readNormEstState), "factor_status": the factor's (Solver.readFactorStatus)} as device
    tensors.  A factor that broke down gives a non-finite estimate; nothing is read back.  Not
    differentiable."""
    what = "cond_estimate"
    v = _detached(pattern, values, what)
    _ag._check_device(pattern.solver, what, v)
    sol = pattern.solver
    batched = v.dim() == 2
    with _OnCurrentStream(sol, v.device):
        L = pattern.assembly.assemble(v)
        s = _jacobi_scale(pattern, L) if scaled else None
        members = _ag._members(L) if batched else L
        sol.factor(members)
        status = sol.factorStatus(members)
        D = None
        if scaled:  # (S A S)^-1 = D A^-1 D with D = S^-1 = sqrt(diag A)
            D = pattern.toInternal(1.0 / s, 1 if batched else 0).contiguous()
            D = _ag._members(D) if batched else D
        inv, state = sol.invNorm1(members, scale=D, return_state=True)
        est = _norm1(pattern, v, s) * inv
    return (est, {"state": state, "factor_status": status}) if return_info else est


# ---- status of the factor ---------------------------------------------------
def check_positive_definite(pattern, values, damping=None):
    """Assembles and factors A(values), and returns the decoded status of the factor
    (Solver.readFactorStatus: ok, first, param, offsetInParam, count, minDiag, maxDiag) with one more
    key, `scalar`: the CALLER's index of the first failing pivot (None when ok), through the inverse of
    scalarPermutation().  The factor stops being meaningful at the first bad pivot in the solver's
    internal order, so `scalar` is the internally-first failure, not the smallest caller index.  A list
    of dicts for a batch [B, nnz].  With a JacobianPattern, `values` are the Jacobian's, A = J^T J, and
    damping = (alpha, beta) (floats or device tensors) is applied on the device first: diag <- diag (1 +
    alpha) + beta.  Synchronises (it reads 32 bytes per matrix); not differentiable."""
    what = "check_positive_definite"
    jac = isinstance(pattern, JacobianPattern)
    _check_values(pattern, values, what, _Pattern)
    if damping is not None and not jac:
        raise ValueError("%s: damping goes with a JacobianPattern" % what)
    sol = pattern.solver
    v = values.detach().contiguous()
    with _OnCurrentStream(sol, v.device):
        data = pattern.normal_eq.hessian(v) if jac else pattern.assembly.assemble(v)
        members = list(data) if v.dim() == 2 else data
        if damping is not None:
            try:
                alpha, beta = damping
            except (TypeError, ValueError):
                raise TypeError("%s: damping must be a pair (alpha, beta), got %r" % (what, damping)) from None
            sol.dampDiagonal(members, alpha, beta)
        sol.factor(members)
        status = sol.readFactorStatus(sol.factorStatus(members))
    # _to_internal = argsort(scalarPermutation()) is indexed by the INTERNAL scalar and gives the caller's
    for st in status if isinstance(status, list) else [status]:
        st["scalar"] = int(pattern._to_internal[st["first"]]) if st["first"] >= 0 else None
    return status
