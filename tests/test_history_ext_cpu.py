"""CPU: the extended history vocabulary (tests/history_ext.py) leaves the committed walks of tests/history.py
what they were, its own walks cover what they must, the entry lists of every structure reach both kernel forms
of the ordered-sum core, and the harness is shown to catch the two leaks an entry map can have.  No GPU: a fake
solver in the style of tests/test_history_cpu.py runs the walks of EXT_WALK_SEEDS under a vocabulary of the
real operations' names.

The fake map sums its operand in the order of a "device table" (a permutation of its host table, one per form:
the forward calls read it as it is, the adjoint calls reversed).  It has two leaks:
  first_use  the device table is uploaded once, in the form the first caller needs, and handed to the callers
             that need the other form too.
  address    the device tables are cached on the solver by the address of the host table; the cache survives
             map_lifetime, and a new map whose host table lies where an old one lay is served the old table.
Either changes the order of a sum only, which stays inside the tolerance of the fake's own check: only the
bitwise veteran / fresh comparison of run_history can see it."""
import ast
import re

import numpy as np
import pytest

import history as H
import history_ext as X
from test_history_cpu import FakeSolver, TOL, _build, _check, _run, _run_refused

N = 24  # length of a fake map's operand
CALLS = {kind: X.CASES[kind].calls for kind in X.NEW_FAMILIES}


def _host_table(kind, variant):
    return np.random.default_rng(sum(map(ord, kind)) + 7 * variant).permutation(N)


class FakeMap:
    def __init__(self, solver, kind, variant):
        self.solver, self.kind, self.variant = solver, kind, variant
        self.host = _host_table(kind, variant)
        self.address = solver.allocate()
        self.dev = {}

    def close(self):
        self.solver.free.append(self.address)

    def table(self, form):
        upload = lambda: self.host[::-1].copy() if form else self.host.copy()  # noqa: E731
        if self.solver.ext_leak == "first_use":
            return self.dev.setdefault("table", upload())       # LEAK: whatever form the first caller needed
        if self.solver.ext_leak == "address":
            return self.solver.by_address.setdefault((self.address, form), upload())  # LEAK: outlives the map
        return self.dev.setdefault(form, upload())

    def call(self, name, x):
        """out[b] = the elements of x[b] added one by one in the order of the table"""
        order = self.table(CALLS[self.kind].index(name) % 2)
        acc = np.zeros(len(x), dtype=x.dtype)
        for k in order:
            acc = acc + x[:, k]
        return acc


class ExtFake(FakeSolver):
    def __init__(self, leak=None):
        FakeSolver.__init__(self, None)
        self.ext_leak, self.maps, self.free, self.top, self.by_address = leak, {}, [], 0, {}

    def allocate(self):
        """the lowest free address, as an allocator that reuses what was just freed"""
        if self.free:
            self.free.sort()
            return self.free.pop(0)
        self.top += 1
        return self.top - 1

    def map(self, kind, variant):
        if (kind, variant) not in self.maps:
            self.maps[kind, variant] = FakeMap(self, kind, variant)
        return self.maps[kind, variant]

    def drop(self, kind):
        for key in [k for k in self.maps if k[0] == kind]:
            self.maps.pop(key).close()


def _make_fake_op(op):
    kind = op.family

    def build(solver, dtype, batch, nrhs, seed):
        x = np.random.default_rng(seed).standard_normal((batch, N)).astype(dtype)
        order = [CALLS[kind][k] for k in np.random.default_rng(seed).permutation(len(CALLS[kind]))]
        return {"x": x, "dtype": np.dtype(dtype), "variant": (seed // 2) % 2, "order": order}

    def run(solver, i):
        x0 = i["x"].copy()
        m = solver.map(kind, i["variant"])
        out = {name: m.call(name, i["x"]) for name in i["order"]}
        out["_readonly"] = [("x", i["x"], x0)]
        return out

    def check(i, o):
        x = i["x"].astype(np.float64)
        worst = 0.0
        for name in i["order"]:
            err = (np.abs(o[name].astype(np.float64) - x.sum(1)) / np.abs(x).sum(1)).max()
            assert err < TOL[i["dtype"]], (name, err)
            worst = max(worst, err / TOL[i["dtype"]])
        return {"fake": worst}
    return H.Op(op.name, op.family, build, run, check, bitwise=CALLS[kind], uses_batch=op.uses_batch,
                uses_nrhs=op.uses_nrhs)


def _fake_lifetime(solver, i):
    solver.drop(i["kind"])
    return {}


def _fake_vocabulary():
    out = []
    for op in X.EXT_VOCABULARY:
        if op.name == "map_lifetime":
            out.append(H.Op(op.name, op.family, op.build, _fake_lifetime, lambda i, o: {}, control=True))
        elif op.control:
            out.append(H.Op(op.name, op.family, lambda *a: {}, lambda s, i: {}, lambda i, o: {}, control=True))
        elif op.family == "error":
            out.append(H.Op(op.name, op.family, _build, _run_refused, lambda i, o: {}))
        elif op.family in X.NEW_FAMILIES:
            out.append(_make_fake_op(op))
        else:
            out.append(H.Op(op.name, op.family, _build, _run, _check, bitwise=("out",), uses_batch=op.uses_batch,
                            uses_nrhs=op.uses_nrhs))
    return out


FAKE = _fake_vocabulary()
LEAKS = ["first_use", "address"]


def _walks():
    return [(name, seed, steps) for name, ws in X.ext_walks(FAKE).items() for seed, steps in ws]


def _run_fake(steps, leak, **kw):
    return H.run_history(lambda: ExtFake(leak), steps, hooks=H.HostHooks, **kw)


# ---- the base vocabulary and its committed walks are what they were ------------------------------------------

BASE_NAMES = """factor factorUpTo+factorFrom factor.perOp solve solveL solveLt solveLUpTo+solveLFrom
solveLtFrom+solveLtUpTo addMvFrom pseudoFactorFrom selectedInverse+marginals logDet+factorStatus+dampDiagonal
patternGrad+patternOuter factorAdjoint factorAdjointUpTo+schurComplement selectedInverseAdjoint
inverseBlocks+halfInverseColumns refused forcePerOp=1 forcePerOp=0 collectOpStats=1 collectOpStats=0
setStream=second setStream=default""".split()

COMMITTED = {
    ("tail", 5331): """
factorAdjointUpTo+schurComplement:float64:b1:r17:s381048 solveLt:float64:b2:r16:s164017
factorAdjoint:float32:b1:r1:s482026 addMvFrom:float64:b2:r17:s887112 solveLt:float64:b1:r1:s336810
solveLUpTo+solveLFrom:float32:b17:r3:s652893 solve:float64:b17:r8:s913879 factor.perOp:float64:b2:r16:s625476
solveLUpTo+solveLFrom:float32:b2:r3:s907844 selectedInverse+marginals:float64:b5:r17:s954890
inverseBlocks+halfInverseColumns:float32:b2:r16:s388492 logDet+factorStatus+dampDiagonal:float32:b5:r16:s193611
factor.perOp:float32:b2:r8:s52672 patternGrad+patternOuter:float64:b5:r3:s77624
inverseBlocks+halfInverseColumns:float32:b1:r8:s256899 selectedInverse+marginals:float64:b1:r17:s490374
factorUpTo+factorFrom:float64:b17:r8:s630953 pseudoFactorFrom:float64:b2:r3:s565698
patternGrad+patternOuter:float64:b1:r8:s548656 logDet+factorStatus+dampDiagonal:float64:b1:r8:s448071""",
    ("tail", 2530): """
factorAdjoint:float64:b2:r16:s132591 solveL:float32:b17:r8:s10452
selectedInverse+marginals:float64:b5:r1:s583282 factorUpTo+factorFrom:float64:b1:r8:s707340
factorAdjointUpTo+schurComplement:float64:b1:r3:s586714 solveLUpTo+solveLFrom:float64:b2:r8:s892918
factor.perOp:float64:b17:r8:s613750 logDet+factorStatus+dampDiagonal:float32:b5:r8:s103891
selectedInverse+marginals:float32:b17:r16:s337545 forcePerOp=0:float32:b2:r17:s853966
solveLUpTo+solveLFrom:float64:b17:r1:s798923 factorAdjointUpTo+schurComplement:float64:b17:r16:s909288
logDet+factorStatus+dampDiagonal:float32:b1:r3:s212341 factor:float64:b5:r17:s140591
logDet+factorStatus+dampDiagonal:float32:b5:r3:s647580 factorAdjointUpTo+schurComplement:float32:b1:r3:s547709
refused:float32:b17:r3:s893779 solveLtFrom+solveLtUpTo:float64:b2:r1:s547580
patternGrad+patternOuter:float32:b2:r8:s853443 selectedInverse+marginals:float64:b2:r16:s435073""",
    ("tail", 20): """
solveLtFrom+solveLtUpTo:float32:b1:r3:s409168 forcePerOp=1:float32:b1:r17:s694068
logDet+factorStatus+dampDiagonal:float64:b5:r16:s301874 forcePerOp=0:float64:b1:r17:s813305
setStream=second:float32:b1:r3:s467947 refused:float64:b2:r8:s702443 addMvFrom:float32:b5:r17:s136685
factorUpTo+factorFrom:float64:b1:r3:s616210 solveLt:float64:b1:r1:s11333
factorAdjointUpTo+schurComplement:float32:b2:r1:s812174 setStream=default:float32:b2:r8:s697423
collectOpStats=1:float64:b17:r3:s446388 factor:float32:b17:r3:s926281 collectOpStats=0:float32:b1:r1:s561650
logDet+factorStatus+dampDiagonal:float64:b2:r17:s607320 refused:float32:b5:r1:s375404
selectedInverse+marginals:float64:b2:r1:s427300 factorUpTo+factorFrom:float64:b1:r16:s374527
refused:float64:b1:r8:s377542 factorAdjointUpTo+schurComplement:float64:b1:r8:s357791""",
    ("sweep", 503): """
selectedInverse+marginals:float64:b5:r8:s403649 refused:float64:b17:r3:s422896
inverseBlocks+halfInverseColumns:float32:b1:r16:s985999 setStream=default:float64:b1:r16:s631579
addMvFrom:float64:b2:r17:s371770 factorAdjoint:float64:b1:r1:s898080
logDet+factorStatus+dampDiagonal:float64:b5:r3:s515150 inverseBlocks+halfInverseColumns:float64:b17:r16:s760719
patternGrad+patternOuter:float32:b1:r1:s299061 selectedInverse+marginals:float32:b5:r16:s478814
addMvFrom:float32:b1:r3:s915610 inverseBlocks+halfInverseColumns:float64:b17:r1:s973575
selectedInverseAdjoint:float32:b1:r1:s834718 inverseBlocks+halfInverseColumns:float64:b1:r3:s453980
solveL:float32:b1:r8:s902556 logDet+factorStatus+dampDiagonal:float64:b2:r17:s634605
solveLtFrom+solveLtUpTo:float32:b2:r16:s766651 factor:float32:b1:r1:s865050
selectedInverse+marginals:float32:b1:r17:s489256 logDet+factorStatus+dampDiagonal:float32:b5:r3:s883129""",
    ("sweep", 1): """
logDet+factorStatus+dampDiagonal:float32:b17:r17:s249229 solveLUpTo+solveLFrom:float64:b17:r16:s549594
setStream=default:float64:b5:r17:s329732 solve:float32:b17:r1:s383312
selectedInverse+marginals:float64:b1:r16:s62021 solveLUpTo+solveLFrom:float64:b17:r1:s724790
refused:float32:b1:r3:s969925 solveLUpTo+solveLFrom:float32:b2:r16:s362851
patternGrad+patternOuter:float64:b5:r8:s872095 collectOpStats=1:float64:b5:r17:s214844
logDet+factorStatus+dampDiagonal:float64:b2:r8:s673682 selectedInverse+marginals:float32:b2:r17:s69016
selectedInverseAdjoint:float32:b1:r3:s191324 forcePerOp=0:float32:b17:r17:s876537
logDet+factorStatus+dampDiagonal:float64:b1:r17:s645721 pseudoFactorFrom:float32:b2:r3:s692541
patternGrad+patternOuter:float32:b17:r1:s42207 selectedInverse+marginals:float64:b2:r8:s890878
factorUpTo+factorFrom:float64:b17:r8:s885520 addMvFrom:float64:b17:r3:s871668""",
    ("bipartite", 409): """
pseudoFactorFrom:float64:b1:r16:s190973 setStream=second:float64:b1:r17:s550638 solveLt:float32:b1:r16:s269829
patternGrad+patternOuter:float64:b5:r3:s487262 solveLt:float32:b2:r8:s694900
pseudoFactorFrom:float32:b5:r1:s235174 logDet+factorStatus+dampDiagonal:float64:b1:r8:s298078
patternGrad+patternOuter:float64:b1:r16:s206147 factorUpTo+factorFrom:float32:b1:r1:s267141
inverseBlocks+halfInverseColumns:float32:b1:r3:s416816 selectedInverse+marginals:float32:b1:r17:s25792
factor.perOp:float64:b5:r3:s91179 solve:float32:b2:r1:s699686
inverseBlocks+halfInverseColumns:float64:b1:r17:s805207 solveLUpTo+solveLFrom:float64:b2:r16:s844645
logDet+factorStatus+dampDiagonal:float32:b17:r8:s3609 factor:float64:b1:r3:s556220
logDet+factorStatus+dampDiagonal:float64:b17:r8:s211440 solve:float32:b1:r1:s438983
addMvFrom:float64:b17:r3:s16088""",
    ("bipartite", 2): """
solveLUpTo+solveLFrom:float64:b17:r3:s600100 refused:float32:b1:r8:s274970
solveLtFrom+solveLtUpTo:float64:b5:r8:s678712 factorAdjoint:float64:b5:r17:s683065 factor:float32:b2:r8:s692459
refused:float64:b17:r17:s223786 selectedInverse+marginals:float32:b2:r1:s957825 solveL:float32:b5:r8:s644436
patternGrad+patternOuter:float32:b2:r8:s862118 selectedInverse+marginals:float32:b17:r1:s829356
factor.perOp:float64:b5:r8:s56888 forcePerOp=0:float32:b2:r16:s579258
logDet+factorStatus+dampDiagonal:float32:b2:r3:s693448 refused:float32:b5:r8:s362927
solveL:float32:b1:r1:s112633 setStream=default:float64:b17:r3:s450585
patternGrad+patternOuter:float64:b5:r8:s937343 factorUpTo+factorFrom:float64:b1:r8:s549451
refused:float64:b17:r8:s96458 factorUpTo+factorFrom:float64:b17:r1:s12832""",
    ("range", 4412): """
selectedInverseAdjoint:float64:b5:r17:s166775 patternGrad+patternOuter:float64:b1:r17:s475973
selectedInverseAdjoint:float32:b1:r1:s339848 solve:float64:b2:r17:s173628
patternGrad+patternOuter:float32:b1:r3:s871990 addMvFrom:float64:b1:r17:s475196
setStream=second:float32:b2:r1:s942395 factor:float64:b2:r1:s894035
selectedInverse+marginals:float32:b17:r17:s123849 factorAdjoint:float32:b2:r17:s64085
solveLUpTo+solveLFrom:float64:b5:r16:s304004 addMvFrom:float32:b5:r8:s949831
selectedInverse+marginals:float64:b1:r3:s270385 patternGrad+patternOuter:float64:b1:r17:s844023
solveLUpTo+solveLFrom:float32:b1:r16:s177594 selectedInverse+marginals:float32:b17:r1:s653770
forcePerOp=0:float64:b1:r3:s880060 forcePerOp=1:float64:b17:r8:s620243
selectedInverseAdjoint:float32:b2:r16:s904097 factorUpTo+factorFrom:float64:b5:r17:s51033""",
    ("range", 3): """
factor:float32:b17:r1:s94129 patternGrad+patternOuter:float64:b2:r16:s734577
collectOpStats=1:float64:b1:r8:s430628 solveLt:float64:b5:r3:s319989
patternGrad+patternOuter:float32:b17:r1:s76917 refused:float64:b1:r17:s662664
logDet+factorStatus+dampDiagonal:float64:b2:r1:s254415 factorAdjoint:float64:b1:r8:s931463
logDet+factorStatus+dampDiagonal:float32:b5:r8:s741756 patternGrad+patternOuter:float32:b1:r17:s657652
solveLtFrom+solveLtUpTo:float64:b17:r16:s325602 setStream=default:float64:b5:r3:s902186
logDet+factorStatus+dampDiagonal:float64:b5:r3:s628710 inverseBlocks+halfInverseColumns:float64:b1:r3:s128954
logDet+factorStatus+dampDiagonal:float32:b1:r16:s181373 selectedInverseAdjoint:float64:b17:r3:s850901
inverseBlocks+halfInverseColumns:float64:b17:r17:s606884 logDet+factorStatus+dampDiagonal:float64:b5:r17:s54094
factor:float32:b5:r3:s626810 inverseBlocks+halfInverseColumns:float64:b2:r8:s305774""",
    ("widths", 6819): """
patternGrad+patternOuter:float32:b2:r8:s525024 logDet+factorStatus+dampDiagonal:float32:b17:r17:s790877
pseudoFactorFrom:float64:b17:r16:s266539 solve:float32:b1:r3:s620837
inverseBlocks+halfInverseColumns:float32:b1:r3:s248769 patternGrad+patternOuter:float32:b17:r16:s739937
selectedInverse+marginals:float64:b1:r3:s786728 addMvFrom:float32:b17:r1:s331220
solveLtFrom+solveLtUpTo:float64:b1:r16:s759581 inverseBlocks+halfInverseColumns:float64:b17:r1:s7887
factorUpTo+factorFrom:float32:b17:r3:s111757 factorAdjoint:float32:b2:r17:s490203
selectedInverse+marginals:float64:b5:r16:s893430 solve:float32:b5:r3:s521667
factorAdjoint:float64:b17:r8:s578669 selectedInverse+marginals:float32:b17:r17:s679471
solveLUpTo+solveLFrom:float64:b5:r3:s763796 refused:float32:b2:r16:s138612 solveLt:float64:b2:r17:s183090
forcePerOp=0:float64:b1:r1:s918292""",
    ("widths", 6): """
logDet+factorStatus+dampDiagonal:float32:b5:r3:s449915 refused:float32:b5:r3:s672285
patternGrad+patternOuter:float64:b17:r17:s846268 factorUpTo+factorFrom:float64:b17:r1:s48084
logDet+factorStatus+dampDiagonal:float32:b17:r8:s627468 inverseBlocks+halfInverseColumns:float64:b1:r17:s759466
factor:float64:b1:r1:s947982 selectedInverse+marginals:float32:b2:r8:s813632
inverseBlocks+halfInverseColumns:float32:b2:r17:s229800 solveLUpTo+solveLFrom:float64:b1:r8:s881289
collectOpStats=0:float64:b17:r16:s894714 setStream=second:float64:b1:r8:s436850
setStream=default:float64:b5:r17:s973624 selectedInverse+marginals:float64:b1:r8:s91810
factorAdjointUpTo+schurComplement:float32:b1:r8:s248355 inverseBlocks+halfInverseColumns:float32:b1:r8:s81823
solveL:float32:b17:r1:s767444 logDet+factorStatus+dampDiagonal:float32:b17:r17:s397569
factor:float32:b5:r3:s193129 inverseBlocks+halfInverseColumns:float32:b2:r17:s213843""",
}


def test_the_base_vocabulary_is_a_prefix_and_the_committed_walks_are_what_they_were():
    names = [op.name for op in X.EXT_VOCABULARY]
    assert names[:len(BASE_NAMES)] == BASE_NAMES == [op.name for op in H.VOCABULARY]
    assert X.EXT_VOCABULARY[:len(H.VOCABULARY)] == H.VOCABULARY, "the base operations are not the same objects"
    assert len(set(names)) == len(names)
    assert [op.family for op in X.EXT_OPS] == list(X.NEW_FAMILIES) + ["control"] and X.EXT_OPS[-1].control
    walks = H.committed_walks()
    assert {(n, s) for n, ws in walks.items() for s, _ in ws} == set(COMMITTED)
    for name, ws in walks.items():
        for seed, steps in ws:
            assert H.describe(steps) == COMMITTED[name, seed].split(), (name, seed)


def test_the_fake_vocabulary_gets_the_walks_of_the_real_one():
    real, fake = X.ext_walks(), X.ext_walks(FAKE)
    assert set(real) == set(H.STRUCTURES) == set(X.EXT_WALK_SEEDS)
    for name in real:
        assert len(real[name]) >= 2
        for (s0, a), (s1, b) in zip(real[name], fake[name]):
            assert s0 == s1 and H.describe(a) == H.describe(b) and len(a) == X.EXT_WALK_LENGTH == 20
    steps = real["tail"][0][1]
    assert H.describe(H.parse(X.EXT_VOCABULARY, H.describe(steps))) == H.describe(steps)


def test_ext_seeds_cover_every_pair_with_a_new_family_and_every_change():
    walks = X.ext_walks()
    everything = [steps for ws in walks.values() for _, steps in ws]
    assert {op.family for op in X.EXT_OPS if not op.control} == set(X.NEW_FAMILIES)
    assert X.missing_pairs(everything) == []
    for name, ws in walks.items():
        mine = [steps for _, steps in ws]
        assert [m for m in H.missing_coverage(mine, X.FAMILIES) if m[0] != "pair"] == [], name
        ops = [s.op.name for steps in mine for s in steps]
        assert any(n.startswith("setStream") for n in ops), name
        # a map is used, dropped by map_lifetime and used again
        reused = False
        for steps in mine:
            used, dropped = set(), set()
            for s in steps:
                if s.op.name == "map_lifetime":
                    kind = X.MAP_KINDS[s.seed % len(X.MAP_KINDS)]
                    dropped |= {kind} & used
                elif s.op.family in X.MAP_KINDS:
                    reused |= s.op.family in dropped
                    used.add(s.op.family)
        assert reused, name
    ops = {s.op.name for steps in everything for s in steps}
    assert {op.name for op in X.EXT_OPS} <= ops, "a new operation never occurs"


@pytest.mark.parametrize("name", list(H.STRUCTURES))
def test_entry_lists_reach_both_kernel_forms(name):
    """the lists are what history_ext says they are, and the maps built from them (host work only) have long
    runs besides the tiles: both forms of the ordered-sum core run"""
    S = H.STRUCTURES[name]
    sol = S.host
    rows, cols = X.sym_list(S)
    n = sol.order()
    low = rows >= cols
    counts = np.unique(rows[low] * n + cols[low], return_counts=True)[1]
    assert (~low).any() and (counts > 1).any() and 65 in counts and 129 in counts
    assert len(counts) < int((S.coords[0] >= S.coords[1]).sum()), "every stored element receives an entry"
    for variant in ("lower", "full"):
        c = X.case(S, "assembly", variant)
        info = c.make(sol).info()
        assert info["long_runs"] >= 2 and info["tiles"] > 0 and info["max_run"] == 129, info
        assert info["kept"] == int(low.sum()) and info["nnz"] == (len(rows) if variant == "full" else info["kept"])
        p = X.case(S, "sym_product", variant).make(sol).info()
        assert p["long_rows"] > 0 and p["kept"] == info["kept"], p
    jr, jc, m = X.jac_list(S)
    assert len(set(zip(jr.tolist(), jc.tolist()))) == len(jr) and jr.max() == m - 1 and 3 not in jr
    info = X.case(S, "normal_eq").make(sol).info()
    assert info["long_runs"] > 0 and info["tiles"] > 0 and info["max_run"] > 64, info


# ---- the two leaks ---------------------------------------------------------------------------------------------

def test_the_clean_fake_passes_every_ext_walk():
    report = {}
    for name, seed, steps in _walks():
        _run_fake(steps, None, tag="%s/%d" % (name, seed), report=report)
    assert set(X.NEW_FAMILIES) <= set(report) and all({"veteran", "fresh"} <= set(v) for v in report.values())


@pytest.mark.parametrize("leak", LEAKS)
def test_each_leak_fails_and_the_message_reproduces_it(leak):
    caught = {}
    for name, seed, steps in _walks():
        with_leak = None
        try:
            _run_fake(steps, leak, tag="%s/%d" % (name, seed))
        except H.HistoryError as e:
            with_leak = str(e)
        if with_leak is None:
            continue
        caught.setdefault(name, []).append(seed)
        m = re.search(r"history %s/%d: the veteran / fresh comparison failed at step (\d+) \(([^)]*)\)" % (name, seed),
                      with_leak)
        assert m, with_leak
        k = int(m.group(1))
        lines = ast.literal_eval(re.search(r"steps so far: (\[.*\])", with_leak).group(1))
        assert len(lines) == k + 1 and lines[-1] == m.group(2) and lines == H.describe(steps[:k + 1])
        assert steps[k].op.family in X.NEW_FAMILIES
        # the message reproduces the failure by itself: the same step fails, and nothing before it does
        again = H.parse(FAKE, lines)
        with pytest.raises(H.HistoryError, match=r"failed at step %d " % k):
            _run_fake(again, leak)
        _run_fake(again[:-1], leak)
    print(leak, caught)
    assert set(caught) == set(X.EXT_WALK_SEEDS), (leak, caught)


@pytest.mark.parametrize("leak", LEAKS)
def test_the_leaks_pass_without_the_comparison(leak):
    """the leaks stay inside the check's tolerance on veteran and fresh alike: with compare=False run_history
    passes them"""
    for name, seed, steps in _walks():
        _run_fake(steps, leak, compare=False)
