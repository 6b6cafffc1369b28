"""History independence of the entry maps, the factor products and the BAL pipeline: the extension of
tests/history.py that tests/test_history_ext_gpu.py and tests/test_history_ext_cpu.py run.

An entry map (Assembly, NormalEquations, SymProduct) owns its device tables, each uploaded by the first call
that asks for it (csrc/hip_extensions.hip, HipEntryMapDev), stages batched pointers through its Solver's ring
of 32 slots and launches on the stream the Solver holds at call time; mulL / mulLt build their plan on first
use.  The operations here keep the maps of a veteran Solver in solver._ext[(kind, variant)], so that one map
object lives through a whole history, while a fresh Solver builds its own; every result is compared bitwise
with the numpy restatement of its owning test (assembly_ref, normal_eq_ref, sym_product_ref) or, for the
factor products, held to the element-wise bound of factor_product_ref, and the veteran's bits must be the
fresh Solver's.

EXT_VOCABULARY is history.VOCABULARY, unchanged and first, then the new operations: history.random_history
depends on the names and order of a vocabulary, so the committed walks of history.WALK_SEEDS stay what they
were and EXT_WALK_SEEDS names walks of their own.

A Case is one kind of map on one Structure with one fixed entry list: make(solver) builds the map,
inputs() draws host operands, run() one call (a batch, or one member alone) on new device tensors into
outputs full of NaN, want() the numpy restatement of one member.  Nothing here touches the GPU at import."""
import gc

import numpy as np

import assembly_ref as AR
import factor_product_ref as FP
import history as H
import normal_eq_ref as NR
import sym_product_ref as SR
from history import F32, F64, Op, Step, Structure  # noqa: F401  (re-exported for the tests)

NEW_FAMILIES = ("assembly", "normal_eq", "sym_product", "factor_product")
FAMILIES = H.REQUIRED_FAMILIES + NEW_FAMILIES
MAP_KINDS = ("assembly", "normal_eq", "sym_product")
LONG_RUN = 64  # the long-run criterion of csrc/entry_map.h: runs of more terms are summed by a whole wave


# ---- the entry lists of a structure ----------------------------------------------------------------------

def _to_user(S):
    """to_user[internal scalar] = the caller's scalar"""
    return S.cached("ext_to_user", lambda: np.argsort(S.host.scalarPermutation()))


def _rng(S, salt):
    return np.random.default_rng(sum(map(ord, S.name)) + salt)


def sym_list(S):
    """(rows, cols) of the symmetric entry list of a structure, in the caller's order: up to 260 stored lower
    elements (20 of them diagonal) split into 1..4 contributions each, about 30 % of the off-diagonal ones
    mirrored into the upper triangle (triangle "full" skips those; the "lower" list is this one without them),
    one more element with exactly 65 entries and one with exactly 129, shuffled.  Every other stored element
    receives no entry."""
    def make():
        rng = _rng(S, 1)
        ci, cj = S.coords
        tu = _to_user(S)
        low = np.nonzero(ci > cj)[0]
        diag = np.nonzero(ci == cj)[0]
        pick = np.concatenate([rng.choice(low, size=min(len(low) // 2, 242), replace=False),
                               rng.choice(diag, size=min(len(diag) // 2, 20), replace=False)])
        i, j = tu[ci[pick]], tu[cj[pick]]
        r, c = np.maximum(i, j).astype(np.int64), np.minimum(i, j).astype(np.int64)
        assert len(set(zip(r.tolist(), c.tolist()))) == len(r)
        rows, cols, _ = AR.duplicated(r[2:], c[2:], rng, max_dup=4, full=True)
        rows = np.concatenate([rows, np.full(LONG_RUN + 1, r[0]), np.full(2 * LONG_RUN + 1, r[1])])
        cols = np.concatenate([cols, np.full(LONG_RUN + 1, c[0]), np.full(2 * LONG_RUN + 1, c[1])])
        order = rng.permutation(len(rows))
        rows, cols = rows[order], cols[order]
        assert (rows < cols).any() and len(pick) < len(low) + len(diag)
        counts = np.unique(rows[rows >= cols] * S.host.order() + cols[rows >= cols], return_counts=True)[1]
        assert (counts == LONG_RUN + 1).sum() >= 1 and (counts == 2 * LONG_RUN + 1).sum() >= 1
        return rows, cols
    return S.cached("ext_sym_list", make)


def jac_list(S):
    """(rows, cols, m) of the Jacobian pattern of a structure, in the caller's order: every row holds 2..6
    scalars of the two params of one stored block (J^T J then stays inside the structure), 70 rows hold the
    same two scalars (three destinations of 70 pairs each, more than the 64 of the long-run criterion), row 3
    is empty; entries shuffled, no position repeated."""
    def make():
        rng = _rng(S, 2)
        ci, cj = S.coords
        tu = _to_user(S)
        ss = np.asarray(S.host.skel()["spanStart"], dtype=np.int64)
        low = np.nonzero(ci >= cj)[0]
        pick = rng.choice(low, size=min(len(low), 40), replace=False)
        sr = np.searchsorted(ss, ci[pick], side="right") - 1
        sc = np.searchsorted(ss, cj[pick], side="right") - 1
        sets, long_pair = [], None
        for a, b in sorted(set(zip(sr.tolist(), sc.tolist()))):
            scalars = np.unique(np.concatenate([np.arange(ss[a], ss[a + 1]), np.arange(ss[b], ss[b + 1])]))
            if long_pair is None and len(scalars) >= 2:
                long_pair = rng.choice(scalars, size=2, replace=False)
            for _ in range(int(rng.integers(1, 4))):
                sets.append(rng.choice(scalars, size=min(len(scalars), int(rng.integers(2, 7))), replace=False))
        assert long_pair is not None
        sets += [long_pair] * (LONG_RUN + 6)
        ids = np.array([k if k < 3 else k + 1 for k in range(len(sets))], dtype=np.int64)  # (row 3 stays empty)
        rows = np.concatenate([np.full(len(s), ids[k]) for k, s in enumerate(sets)])
        cols = tu[np.concatenate(sets)].astype(np.int64)
        order = rng.permutation(len(rows))
        return rows[order], cols[order], len(sets) + 1
    return S.cached("ext_jac_list", make)


# ---- cases: one kind of map on one structure ------------------------------------------------------------------

def _nan(shape, dtype):
    import torch
    return torch.full(tuple(shape), float("nan"), dtype=torch.float64 if np.dtype(dtype) == F64 else torch.float32,
                      device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Case:
    """kind, calls: the names of the map's device calls, the "natural" first one first.  spec(call, i) ->
    (method, operand names, shape of one member's output)"""
    kind, calls = None, ()

    def __init__(self, S, variant=None, lists=None):
        self.S, self.variant, self.host = S, variant, S.host

    def make(self, solver):
        raise NotImplementedError

    def operands(self, rng, m, q, dtype):
        raise NotImplementedError

    def inputs(self, dtype, seed, batch=1, q=1, members=None):
        """host operands of `batch` members, min(batch, 3) of them distinct (member b holds those of
        b % m) unless `members` says otherwise"""
        m = min(batch, 3) if members is None else members
        i = {"dtype": np.dtype(dtype), "batch": batch, "q": q, "m": m, "want": {}}
        i.update(self.operands(np.random.default_rng(seed), m, q, np.dtype(dtype).type))
        return i

    def stage(self, call, i, sel=None):
        """new device tensors for `call` on the whole batch (a single call when it has one member) or on
        member `sel` alone, the output full of NaN: everything launch() needs, so that a test can upload
        first and queue the launches without touching the host in between"""
        method, names, shape = self.spec(call, i)
        idx = list(range(i["batch"])) if sel is None else [sel]
        single = len(idx) == 1
        host = [i[n][idx[0] % i["m"]] if single else np.stack([i[n][b % i["m"]] for b in idx]) for n in names]
        return {"method": method, "dev": [H._dev(h) for h in host], "single": single,
                "out": _nan(shape if single else (len(idx),) + tuple(shape), i["dtype"]),
                "readonly": list(zip(names, host))}

    def launch(self, m, st):
        """-> one output tensor per member"""
        got = getattr(m, st["method"])(*st["dev"], out=st["out"])
        assert got is st["out"]
        return [got] if st["single"] else list(got.unbind(0))

    def run(self, m, call, i, sel=None):
        """stage() and launch(): -> (one output tensor per member, [(name, device operand, host operand)])"""
        st = self.stage(call, i, sel)
        outs = self.launch(m, st)
        return outs, [(n, d, h) for (n, h), d in zip(st["readonly"], st["dev"])]

    def want(self, call, i, b):
        """the numpy restatement of member b (computed once per distinct member)"""
        key = (call, b % i["m"])
        if key not in i["want"]:
            i["want"][key] = self.restate(call, i, b % i["m"])
        return i["want"][key]

    def check(self, call, i, outs, sel=None):
        """every member bitwise its restatement; -> {metric: error / tolerance}"""
        idx = list(range(i["batch"])) if sel is None else [sel]
        assert len(outs) == len(idx)
        for b, o in zip(idx, outs):
            o = np.asarray(o)
            assert not np.isnan(o).any(), (self.kind, call, "member %d: an element was not written" % b)
            assert same_bits(o, self.want(call, i, b)), (self.kind, self.variant, call, "member %d of %d is not "
                                                         "bitwise the numpy restatement" % (b, i["batch"]))
        return {self.kind + "_bits": 0.0}


class AssemblyCase(Case):
    kind, calls = "assembly", ("assemble", "adjoint")

    def __init__(self, S, variant="lower", lists=None):
        Case.__init__(self, S, variant)
        rows, cols = sym_list(S) if lists is None else lists
        if variant == "lower":
            rows, cols = rows[rows >= cols], cols[rows >= cols]
        self.rows, self.cols, self.nnz, self.ds = rows, cols, len(rows), self.host.dataSize()
        offs = lambda: AR.ref_offsets(self.host, rows, cols, variant)  # noqa: E731
        self.offs = S.cached(("ext_offs", variant), offs) if lists is None else offs()

    def make(self, solver):
        return solver.assembly(self.rows, self.cols, self.variant)

    def operands(self, rng, m, q, t):
        return {"values": rng.uniform(-1, 1, (m, self.nnz)).astype(t), "grad": rng.uniform(-1, 1, (m, self.ds)).astype(t)}

    def spec(self, call, i):
        return {"assemble": ("assemble", ["values"], (self.ds,)), "adjoint": ("adjoint", ["grad"], (self.nnz,))}[call]

    def restate(self, call, i, b):
        t, keep = i["dtype"].type, self.offs >= 0
        if call == "assemble":
            out = np.zeros(self.ds, dtype=t)
            np.add.at(out, self.offs[keep], i["values"][b][keep])
            return out
        return np.where(keep, i["grad"][b][np.maximum(self.offs, 0)], t(0)).astype(t)


class NormalEqCase(Case):
    kind, calls = "normal_eq", ("hessian", "hessianAdjoint", "jtVec", "jVec")

    def __init__(self, S, variant=None, lists=None):
        Case.__init__(self, S, variant)
        self.rows, self.cols, self.m = jac_list(S) if lists is None else lists
        self.nnz, self.ds, self.n = len(self.rows), self.host.dataSize(), self.host.order()
        refs = lambda: (NR.ref_pair_table(self.host, self.rows, self.cols, self.m),  # noqa: E731
                        NR.ref_adjoint_terms(self.host, self.rows, self.cols, self.m))
        self.table, self.terms = S.cached("ext_ne_ref", refs) if lists is None else refs()

    def make(self, solver):
        return solver.normalEquations(self.rows, self.cols, self.m)

    def operands(self, rng, m, q, t):
        return {"values": rng.uniform(-1, 1, (m, self.nnz)).astype(t), "grad": rng.uniform(-1, 1, (m, self.ds)).astype(t),
                "r": rng.uniform(-1, 1, (m, self.m, q)).astype(t), "x": rng.uniform(-1, 1, (m, self.n, q)).astype(t)}

    def spec(self, call, i):
        q = i["q"]
        return {"hessian": ("hessian", ["values"], (self.ds,)),
                "hessianAdjoint": ("hessianAdjoint", ["values", "grad"], (self.nnz,)),
                "jtVec": ("jtVec", ["values", "r"], (self.n, q)), "jVec": ("jVec", ["values", "x"], (self.m, q))}[call]

    def restate(self, call, i, b):
        t, v = i["dtype"].type, i["values"][b]
        if call == "hessian":
            return NR.ref_hessian(self.host, self.table, v, t)
        if call == "hessianAdjoint":
            return NR.ref_adjoint(self.terms, self.nnz, v, i["grad"][b], t)
        if call == "jtVec":
            return NR.ref_jt_vec(self.rows, self.cols, self.n, v, i["r"][b], t)
        return NR.ref_j_vec(self.rows, self.cols, self.m, v, i["x"][b], t)


class SymProductCase(Case):
    kind, calls = "sym_product", ("mv", "outer")

    def __init__(self, S, variant="lower", lists=None):
        Case.__init__(self, S, variant)
        rows, cols = sym_list(S) if lists is None else lists
        if variant == "lower":
            rows, cols = rows[rows >= cols], cols[rows >= cols]
        self.rows, self.cols, self.nnz, self.n = rows, cols, len(rows), self.host.order()

    def make(self, solver):
        return solver.symProduct(self.rows, self.cols, self.variant)

    def operands(self, rng, m, q, t):
        return {"values": rng.uniform(-1, 1, (m, self.nnz)).astype(t), "g": rng.uniform(-1, 1, (m, self.n, q)).astype(t),
                "x": rng.uniform(-1, 1, (m, self.n, q)).astype(t)}

    def spec(self, call, i):
        return {"mv": ("mv", ["values", "x"], (self.n, i["q"])), "outer": ("outer", ["g", "x"], (self.nnz,))}[call]

    def restate(self, call, i, b):
        t = i["dtype"].type
        if call == "mv":
            return SR.mv_model(self.n, self.rows, self.cols, self.variant, i["values"][b], i["x"][b], t)
        return SR.outer_model(self.n, self.rows, self.cols, self.variant, i["g"][b], i["x"][b], t)


class FactorProductCase(Case):
    """mulL / mulLt of the Solver itself on factors that another Solver computed (Structure.provided)"""
    kind, calls = "factor_product", ("mulL", "mulLt")

    def __init__(self, S, variant=None, lists=None):
        Case.__init__(self, S, variant)
        self.n = self.host.order()

    def make(self, solver):
        return solver

    def inputs(self, dtype, seed, batch=1, q=1, members=None, provided=True):
        """provided=False: random data in the layout instead of factors (the products read any data)"""
        i = Case.inputs(self, dtype, seed, batch, q, members)
        if provided:
            i["L"] = [self.S.provided("kf", seed + b, dtype) for b in range(i["m"])]
        else:
            rng = np.random.default_rng(seed + 1)
            i["L"] = [rng.uniform(-1, 1, self.host.dataSize()).astype(dtype) for _ in range(i["m"])]
        return i

    def operands(self, rng, m, q, t):
        return {"x": rng.uniform(-1, 1, (m, q, self.n)).astype(t)}

    def stage(self, call, i, sel=None):
        idx = list(range(i["batch"])) if sel is None else [sel]
        hL, hx = [i["L"][b % i["m"]] for b in idx], [i["x"][b % i["m"]] for b in idx]
        Ls, xs = list(H._dev(np.stack(hL)).unbind(0)), list(H._dev(np.stack(hx)).unbind(0))  # (one upload each)
        outs = list(_nan((len(idx),) + hx[0].shape, i["dtype"]).unbind(0))
        return {"method": call, "L": Ls, "x": xs, "out": outs, "q": i["q"],
                "single": len(idx) == 1, "dev": Ls + xs,
                "readonly": [("L %d" % b, h) for b, h in zip(idx, hL)] + [("x %d" % b, h) for b, h in zip(idx, hx)]}

    def launch(self, m, st):
        one = (lambda v: v[0]) if st["single"] else (lambda v: v)
        getattr(m, st["method"])(one(st["L"]), one(st["x"]), out=one(st["out"]), nRHS=st["q"])
        return st["out"]

    def check(self, call, i, outs, sel=None):
        """the element-wise bound t_i eps s_i of factor_product_ref.check"""
        idx = list(range(i["batch"])) if sel is None else [sel]
        worst = 0.0
        for b, o in zip(idx, outs):
            k = b % i["m"]
            if (call, k) not in i["want"]:
                ref, t, s = FP.reference(self.host, i["L"][k], i["x"][k].T, call == "mulLt")
                i["want"][call, k] = (ref, FP.bound(t, s, i["dtype"]))
            ref, lim = i["want"][call, k]
            got = np.asarray(o).T.reshape(ref.shape)
            assert np.isfinite(got).all(), (call, b, "a result is not finite")
            err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
            assert not (err > lim).any(), (call, b, "outside t eps s", float(err.max()))
            worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0)
        return {call: worst}


CASES = {"assembly": AssemblyCase, "normal_eq": NormalEqCase, "sym_product": SymProductCase,
         "factor_product": FactorProductCase}
VARIANTS = {"assembly": ("lower", "full"), "normal_eq": (None,), "sym_product": ("lower", "full"),
            "factor_product": (None,)}


def case(S, kind, variant=None):
    return S.cached(("ext_case", kind, variant), lambda: CASES[kind](S, variant))


def maps_of(solver):
    if not hasattr(solver, "_ext"):
        solver._ext = {}
    return solver._ext


def map_of(solver, c):
    """the veteran keeps one map per (kind, variant) for its whole history; a fresh Solver builds its own"""
    m = maps_of(solver)
    if (c.kind, c.variant) not in m:
        m[c.kind, c.variant] = c.make(solver)
    return m[c.kind, c.variant]


def call_order(c, seed):
    return [c.calls[k] for k in np.random.default_rng(seed).permutation(len(c.calls))]


# ---- operations ----------------------------------------------------------------------------------------------

def _make_op(kind, uses_nrhs):
    def build(solver, dtype, batch, nrhs, seed):
        S = H._S(solver)
        vs = VARIANTS[kind]
        c = case(S, kind, vs[(seed // 2) % len(vs)])
        q = nrhs if uses_nrhs else (1, 3)[seed % 2]
        return {"case": c, "order": call_order(c, seed), "i": c.inputs(dtype, seed, batch, q)}

    def run(solver, a):
        c = a["case"]
        m = map_of(solver, c)
        out, ro = {}, []
        for call in a["order"]:
            out[call], r = c.run(m, call, a["i"])
            ro += [(call + " " + n, d, h) for n, d, h in r]
        out["_readonly"] = ro
        return out

    def check(a, o):
        return H._merge(*[a["case"].check(call, a["i"], o[call]) for call in a["order"]])
    return build, run, check


def _build_lifetime(solver, dtype, batch, nrhs, seed):
    return {"kind": MAP_KINDS[seed % len(MAP_KINDS)]}


def _run_lifetime(solver, a):
    """drops the Solver's maps of one kind and collects them: the next use builds a new map where the old one
    lay"""
    m = maps_of(solver)
    for key in [k for k in m if k[0] == a["kind"]]:
        del m[key]
    gc.collect()
    return {}


def _ext_ops():
    ops = []
    for kind, name, uses_nrhs in (("assembly", "assemble+adjoint", False),
                                  ("normal_eq", "hessian+hessianAdjoint+jtVec+jVec", False),
                                  ("sym_product", "mv+outer", True), ("factor_product", "mulL+mulLt", True)):
        build, run, check = _make_op(kind, uses_nrhs)
        ops.append(Op(name, kind, build, run, check, bitwise=CASES[kind].calls, uses_batch=True, uses_nrhs=uses_nrhs))
    ops.append(Op("map_lifetime", "control", _build_lifetime, _run_lifetime, H._nothing, control=True))
    return ops


EXT_OPS = _ext_ops()
EXT_VOCABULARY = H.VOCABULARY + EXT_OPS
EXT_BY_NAME = {op.name: op for op in EXT_VOCABULARY}


def ext_steps(*specs):
    """steps from (name, dtype, batch, nrhs, seed) tuples over EXT_VOCABULARY"""
    return [Step(EXT_BY_NAME[n], np.dtype(dt), b, r, s) for n, dt, b, r, s in specs]


# Seeds of the random walks over EXT_VOCABULARY per structure, chosen on the host
# (tests/test_history_ext_cpu.py asserts what they cover: over all structures every ordered pair of families
# with a new family on either side; on each structure both dtype switches, a batch decrease and an nRHS
# decrease)
EXT_WALK_LENGTH = 20
EXT_WALK_SEEDS = {"tail": [29827, 33194, 172], "sweep": [31670, 32913], "bipartite": [8449, 39638], "range": [12510, 92],
                  "widths": [16152, 96]}


def ext_walks(vocabulary=None):
    """{structure name: [(seed, steps)]}"""
    vocabulary = EXT_VOCABULARY if vocabulary is None else vocabulary
    return {name: [(s, H.random_history(s, EXT_WALK_LENGTH, vocabulary)) for s in seeds]
            for name, seeds in EXT_WALK_SEEDS.items()}


def missing_pairs(walks):
    """the ordered pairs of families with a new family on either side that `walks` do not hold"""
    pairs = H.coverage(walks)["pairs"]
    return [(a, b) for a in FAMILIES for b in FAMILIES
            if a != b and (a in NEW_FAMILIES or b in NEW_FAMILIES) and (a, b) not in pairs]
