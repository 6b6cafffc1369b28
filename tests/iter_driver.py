"""A raw driver of the bsp_cg_* and bsp_lanczos_* pieces (DESIGN.md sections 24 and 25) for the buffer-edge and
call-history tests: it issues exactly the piece sequence of cg.CgRun.run and lanczos.LanczosRun.run (check_every
None) through the C entries, single and batched, f32 and f64, on buffers that are ALL the caller's -- nothing is
allocated here -- and calls a hook after every piece.

An operand with one array per member (b, x, r, p, Ap, z, minv, values; v0, w, basis) is given as a list of device
tensors, one per member, or as a numpy array of device addresses (uint64), which is what a batch past the chunk
limit uses; the work areas, state, status and coefficients are plain device addresses.  Whether the single or
the batched entry is called is the caller's choice (`batched`), whatever the number of members.

WRITE_SETS carries, as data, what each piece may write according to the headers (hip_cg_kernels.h,
hip_lanczos_kernels.h, include/baspacho_amd.h -- transcribed from their contracts, not from the kernels' code);
everything else a piece is handed is read-only for it.  Nothing here touches the GPU at import."""
import ctypes
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "baspacho_amd.h")

# piece -> the operands it may write.  "columns": the written vector operands change in the columns of the
# problems that run (stop word 0) when the piece starts, and nowhere else; "note" states the exceptions.
# Operand names: CG b x r p ap z minv values state status work; Lanczos v0 w basis slot coef state work
# ("slot": the output slot of the basis, nothing else of the basis).
WRITE_SETS = {
    # host-only entries: nothing on the device
    "cg_state_words": {"writes": ()},
    "cg_work_bytes": {"writes": ()},
    "cg_precond_info": {"writes": ()},
    "cg_precond_table": {"writes": ()},
    "lanczos_state_words": {"writes": ()},
    "lanczos_work_bytes": {"writes": ()},
    # the conjugate gradient
    "cg_precond_build": {"writes": ("minv", "status", "work"), "note": "status: 2 words per member"},
    "cg_init": {"writes": ("state", "work", "x", "r"),
                "note": "all 12 words of every record; x and r only in the columns of a zero right-hand side, "
                        "where they become 0"},
    "cg_alpha": {"writes": ("state", "work")},
    "cg_update": {"writes": ("x", "r", "state", "work"), "columns": ("x", "r")},
    "cg_precond": {"writes": {0: ("state", "work"), 1: ("z", "state", "work"), 2: ("z", "state", "work")},
                   "columns": ("z",), "note": "kind 0: z is the caller's and only read"},
    "cg_direction": {"writes": ("p",), "columns": ("p",)},
    # the Lanczos recurrence
    "lanczos_init": {"writes": ("slot", "state", "work"), "columns": ("slot",)},
    "lanczos_alpha": {"writes": ("state", "work")},
    "lanczos_project": {"writes": ("work",)},
    "lanczos_update": {"writes": ("w", "work"), "fold": ("state", "coef"),
                       "note": "with fold: the record and the entries j and kmax + j of the problem's coefficients"},
    "lanczos_subtract": {"writes": ("w", "work"), "fold": ("state", "coef"),
                         "note": "with fold: the record and the entries j and kmax + j of the problem's coefficients"},
    "lanczos_normalize": {"writes": ("slot",), "columns": ("slot",)},
}
# the product is the caller's operator, not a piece: SymProduct.mv writes every element of its output
PRODUCT_WRITES = {"cg": ("ap",), "lanczos": ("w",)}


def write_set(piece, kind=None, fold=False):
    """the names a piece may write: `kind` for cg_precond, `fold` for lanczos_update / lanczos_subtract"""
    row = WRITE_SETS[piece]
    w = row["writes"]
    if isinstance(w, dict):
        w = w[kind]
    return tuple(w) + (tuple(row.get("fold", ())) if fold else ())


def exported_pieces(header=HEADER):
    """the names X of every bsp_cg_X / bsp_lanczos_X the public header declares (single, batched and both
    precisions folded into one name)"""
    with open(header) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set()
    for fam, rest in re.findall(r"\bint\s+bsp_(cg|lanczos)_(\w+)\s*\(", text):
        names.add(fam + "_" + re.sub(r"(_batched)?_(f64|f32)$", "", rest))
    return sorted(names)


# ---- arguments -------------------------------------------------------------------------------------------
P, I32, I64, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double


def addresses(operand):
    """the device addresses of an operand's members as a uint64 array"""
    if operand is None:
        return None
    if isinstance(operand, np.ndarray):
        assert operand.dtype == np.uint64 and operand.ndim == 1 and operand.flags["C_CONTIGUOUS"]
        return operand
    out = np.empty(len(operand), dtype=np.uint64)
    for m, t in enumerate(operand):
        assert t.is_contiguous()
        out[m] = t.data_ptr()
    return out


class _Entries:
    """what the two drivers share: the single or the batched entry of a piece, the pointer arguments, the hook"""

    def __init__(self, solver, sfx, nb, batched, hook):
        self.solver, self.lib, self.sfx = solver, solver._lib, sfx
        self.nb, self.batched = int(nb), bool(batched)
        assert self.batched or self.nb == 1
        self.hook = hook
        self._keep = []

    def ptrs(self, operand):
        """the pointer argument of an operand: the member's pointer, or the host array of the members' pointers
        (NULL for None)"""
        if operand is None:
            return None
        a = addresses(operand)
        assert len(a) == self.nb, (len(a), self.nb)
        if not self.batched:
            return P(int(a[0]))
        self._keep.append(a)  # the library stages the pointers during the call; keeping them costs nothing
        return a.ctypes.data_as(P)

    def call(self, name, *args):
        fn = getattr(self.lib, "bsp_" + name + ("_batched_" if self.batched else "_") + self.sfx)
        rc = fn(self.solver._h, *args, *((I32(self.nb),) if self.batched else ()))
        del self._keep[:]
        return rc

    def checked(self, name, *args):
        rc = self.call(name, *args)
        if rc != 0:
            raise RuntimeError(self.lib.bsp_last_error().decode("utf-8", "replace"))

    def done(self, piece, step, **info):
        if self.hook is not None:
            self.hook(piece, step, info)


def product_mv(product, values, x, q, out, nb, batched, sfx):
    """out = A x through bsp_sym_product_mv_*: per-member lists of tensors go through SymProduct.mv with out=
    the caller's view, member by member (a member of a batch is bitwise its single call); address arrays go
    to the C entry"""
    if not isinstance(values, np.ndarray):
        for m in range(nb):
            product.mv(values[m], x[m], out=out[m])
        return
    lib, h = product._lib, product.solver._h
    if batched:
        arrs = [addresses(o) for o in (values, x, out)]
        rc = getattr(lib, "bsp_sym_product_mv_batched_" + sfx)(h, product._h, arrs[0].ctypes.data_as(P),
                                                               arrs[1].ctypes.data_as(P), I64(q),
                                                               arrs[2].ctypes.data_as(P), I32(nb))
    else:
        rc = getattr(lib, "bsp_sym_product_mv_" + sfx)(h, product._h, P(int(values[0])), P(int(x[0])), I64(q),
                                                       P(int(out[0])))
    if rc != 0:
        raise RuntimeError(lib.bsp_last_error().decode("utf-8", "replace"))


# ---- the conjugate gradient ------------------------------------------------------------------------------
class CgPieces(_Entries):
    """The pieces of cg.CgRun.run on the caller's buffers.  ops: dict of the per-member operands b, x, r, p, ap,
    and values (the product's), z and minv where the preconditioner needs them; work / state: device addresses
    (work exactly bsp_cg_work_bytes(n, q) per member); kind: None (plain), 0 (the caller's z: given_z(step) is
    called before every precond piece and must leave z = M^-1 r), 1 (jacobi), 2 (block_jacobi); a built-in
    kind is built first (build_work: bsp_cg_work_bytes(n, 1) per member, status: 2 words per member).
    hook(piece, step, info) runs after every piece and after every product ("mv"); step -1 is the start."""

    def __init__(self, solver, product, sfx, n, q, nb, batched, ops, work, state, kind=None, tol=1e-10, max_steps=6,
                 build_work=None, status=None, given_z=None, hook=None, apply_a=None):
        super().__init__(solver, sfx, nb, batched, hook)
        self.product, self.n, self.q = product, int(n), int(q)
        self.ops, self.kind = ops, kind
        self.plain = kind is None
        self.tol, self.max_steps = float(tol), int(max_steps)
        self.tail = (P(work), P(state))
        self.build_work, self.status, self.given_z = build_work, status, given_z
        self.apply_a = apply_a or (lambda: product_mv(product, ops["values"], ops["p"], self.q, ops["ap"], self.nb,
                                                      self.batched, sfx))
        self.nq = (I64(self.n), I64(self.q))

    def build(self):
        o = self.ops
        self.checked("cg_precond_build", self.product._h, I32(self.kind), self.ptrs(o["values"]), self.ptrs(o["minv"]),
                     P(self.build_work), P(self.status))
        self.done("cg_precond_build", -1, kind=self.kind)

    def init(self):
        o = self.ops
        self.checked("cg_init", *self.nq, self.ptrs(o["b"]), self.ptrs(o["x"]), self.ptrs(o["r"]), F64(self.tol),
                     I64(self.max_steps), I32(1 if self.plain else 0), *self.tail)
        self.done("cg_init", -1)

    def precond(self, step):
        o = self.ops
        if self.kind == 0:
            if self.given_z is not None:
                self.given_z(step)
            self.checked("cg_precond", None, I32(0), *self.nq, None, self.ptrs(o["r"]), self.ptrs(o["z"]), *self.tail)
        else:
            self.checked("cg_precond", self.product._h, I32(self.kind), *self.nq, self.ptrs(o["minv"]),
                         self.ptrs(o["r"]), self.ptrs(o["z"]), *self.tail)
        self.done("cg_precond", step, kind=self.kind)

    def direction(self, step):
        o = self.ops
        if not self.plain:
            self.precond(step)
        self.checked("cg_direction", *self.nq, self.ptrs(o["r"] if self.plain else o["z"]), self.ptrs(o["p"]),
                     I32(1 if self.plain else 0), *self.tail)
        self.done("cg_direction", step)

    def iterate(self, step):
        o = self.ops
        self.apply_a()
        self.done("mv", step)
        self.checked("cg_alpha", *self.nq, self.ptrs(o["p"]), self.ptrs(o["ap"]), *self.tail)
        self.done("cg_alpha", step)
        self.checked("cg_update", *self.nq, self.ptrs(o["p"]), self.ptrs(o["ap"]), self.ptrs(o["x"]), self.ptrs(o["r"]),
                     I32(1 if self.plain else 0), *self.tail)
        self.done("cg_update", step)
        self.direction(step)

    def run(self):
        if self.kind in (1, 2):
            self.build()
        self.init()
        self.direction(-1)
        for step in range(self.max_steps):
            self.iterate(step)
        return self


# ---- the Lanczos recurrence ------------------------------------------------------------------------------
class LanczosPieces(_Entries):
    """The pieces of lanczos.LanczosRun.run on the caller's buffers.  ops: dict of the per-member operands v0, w,
    basis (the member's slot 0; slot s lies s slot_stride elements behind) and values (the product's); coef /
    work / state: device addresses (work exactly bsp_lanczos_work_bytes(n, q, kmax) per member); full: full
    reorthogonalisation (kmax slots); else the plain recurrence on `slots` slots, 2 (a ring) or kmax (kept).
    slot_view(m, s): the [n, q] tensor of slot s of member m, for the product (lists of tensors only);
    hook(piece, step, info) runs after every piece and after every product ("mv")."""

    def __init__(self, solver, product, sfx, n, q, kmax, nb, batched, ops, slot_stride, slots, coef, work, state,
                 full=True, breakdown=None, itemsize=None, hook=None, slot_view=None):
        super().__init__(solver, sfx, nb, batched, hook)
        self.product, self.n, self.q, self.kmax = product, int(n), int(q), int(kmax)
        self.ops, self.full = ops, bool(full)
        self.slot_stride, self.slots = int(slot_stride), int(slots)
        self.kept = self.slots >= self.kmax
        assert self.kept or (not self.full and self.slots == min(2, self.kmax))
        self.itemsize = itemsize or (8 if sfx == "f64" else 4)
        self.breakdown = 64.0 * float(np.finfo(np.float64 if sfx == "f64" else np.float32).eps) \
            if breakdown is None else float(breakdown)
        self.head = (I64(self.n), I64(self.q), I64(self.kmax))
        self.coef, self.tail = P(coef), (P(work), P(state))
        self.slot_view = slot_view

    def _basis(self):
        return (self.ptrs(self.ops["basis"]), I64(self.slot_stride), I64(self.slots))

    def _slot(self, j):
        return j if self.kept else j % 2

    def piece(self, name, vec, *args):
        self.checked("lanczos_" + name, *self.head, self.ptrs(vec), *self._basis(), *args, *self.tail)

    def apply_a(self, j):
        o, s = self.ops, self._slot(j)
        if isinstance(o["basis"], np.ndarray):
            x = addresses(o["basis"]) + np.uint64(s * self.slot_stride * self.itemsize)
        else:
            x = [self.slot_view(m, s) for m in range(self.nb)]
        product_mv(self.product, o["values"], x, self.q, o["w"], self.nb, self.batched, self.sfx)

    def init(self):
        self.piece("init", self.ops["v0"], I64(0), F64(self.breakdown))
        self.done("lanczos_init", -1, slot=0)

    def iterate(self, j):
        w = self.ops["w"]
        self.apply_a(j)
        self.done("mv", j)
        self.piece("alpha", w, I64(self._slot(j)))
        self.done("lanczos_alpha", j)
        fold = 0 if self.full else 1
        self.piece("update", w, I64(self._slot(j)), I64(self._slot(max(j - 1, 0))), I32(fold), self.coef)
        self.done("lanczos_update", j, fold=bool(fold))
        if self.full:
            for last in (0, 1):
                self.piece("project", w, I64(j + 1))
                self.done("lanczos_project", j)
                self.piece("subtract", w, I64(j + 1), I32(last), self.coef)
                self.done("lanczos_subtract", j, fold=bool(last))
        if j + 1 < self.kmax:
            self.piece("normalize", w, I64(self._slot(j + 1)))
            self.done("lanczos_normalize", j, slot=self._slot(j + 1))

    def run(self):
        self.init()
        for j in range(self.kmax):
            self.iterate(j)
        return self


def work_bytes(solver, family, n, q, kmax=None):
    """bsp_cg_work_bytes / bsp_lanczos_work_bytes"""
    need = I64(0)
    if family == "cg":
        rc = solver._lib.bsp_cg_work_bytes(solver._h, I64(n), I64(q), ctypes.byref(need))
    else:
        rc = solver._lib.bsp_lanczos_work_bytes(solver._h, I64(n), I64(q), I64(kmax), ctypes.byref(need))
    if rc != 0:
        raise RuntimeError(solver._lib.bsp_last_error().decode("utf-8", "replace"))
    return int(need.value)
