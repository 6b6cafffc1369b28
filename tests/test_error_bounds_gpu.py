"""GPU: the error bounds of DESIGN.md section 23 on the MI355X.  residual, absMv, maxRatio and colMax must be
bitwise their numpy statements (error_bounds_ref.py) on the shapes where each kernel path can go wrong, on
framed buffers at odd element offsets; invNorm1 must lie in [true / 3, true (1 + n kappa_1 eps)] of the
explicit inverse and follow the restatement's trace wherever that trace is not fragile; cond_estimate, norm1
and solve_refined's tol / return_info are checked through baspacho_amd.sparse; every refusal is raised before
any launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import sparse as S
from assembly_ref import dense_user
from buffer_edges import SENTINEL, framed, is_sentinel
import error_bounds_ref as E
import sym_product_ref as R

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
QS = [1, 2, 3, 16, 17]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dev(a, npdt=None):
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a if npdt is None else a.astype(npdt))).cuda()


def _framed(npdt, ins, out_shapes, call):
    """call(*inputs, *outs) with every tensor a payload of one frame at an odd element offset: inputs
    untouched, guards intact, every out (full of the sentinel before) fully written.  Host copies of outs"""
    outs = [np.full(int(np.prod(s)), SENTINEL[npdt], dtype=npdt) for s in out_shapes]
    fr = framed(npdt, list(ins) + outs)
    args = [fr.view(k).view(h.shape) for k, h in enumerate(ins)]
    os_ = [fr.view(len(ins) + k).view(tuple(s)) for k, s in enumerate(out_shapes)]
    assert all(a.data_ptr() % 16 != 0 for a in args + os_ if a.numel())
    call(*args, *os_)
    torch.cuda.synchronize()
    fr.assert_intact(read_only=range(len(ins)))
    got = [fr.host(len(ins) + k).reshape(s) for k, s in enumerate(out_shapes)]
    for g in got:
        assert not is_sentinel(g).any(), "%d elements of an output were not written" % int(is_sentinel(g).sum())
    return got


# ---- residual, absMv ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", R.CASES)
def test_residual_and_abs_mv_bitwise(name, dt):
    _, npdt = DT[dt]
    c, prod = R.case(name), R.pattern(name).product
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    rng = np.random.default_rng(41)
    v = c["values"].astype(npdt)
    for q in [None] + QS:
        x = rng.uniform(-1, 1, (n,) if q is None else (n, q)).astype(npdt)
        b = rng.uniform(-1, 1, x.shape).astype(npdt)
        wr, wd = E.residual_model(n, rows, cols, tri, v, x, b, npdt)
        r, d = _framed(npdt, [v, x, b], [x.shape, x.shape],
                       lambda a, xx, bb, ro, do: prod.residual(a, xx, bb, out=(ro, do)))
        assert _bits_equal(r, wr) and _bits_equal(d, wd), (name, dt, q)
        mv = prod.mv(_dev(v), _dev(x)).cpu().numpy()
        assert _bits_equal(r, (b - mv).astype(npdt)), "r is not bitwise b - mv"
        (t,) = _framed(npdt, [v, x], [x.shape], lambda a, xx, o: prod.absMv(a, xx, out=o))
        assert _bits_equal(t, E.residual_model(n, rows, cols, tri, v, x, None, npdt)[1]), (name, dt, q)
        r2, d2 = prod.residual(_dev(v), _dev(x), _dev(b))
        assert _bits_equal(r2.cpu().numpy(), r) and _bits_equal(d2.cpu().numpy(), d), "two runs differ"


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["dups", "full", "arrow65", "arrow129", "empty"])
def test_residual_batches_bitwise(name, dt):
    _, npdt = DT[dt]
    c, prod = R.case(name), R.pattern(name).product
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    rng = np.random.default_rng(42)
    for nb, q in ((1, 3), (2, None), (2, 17), (5, 1), (5, 16)):
        v = rng.uniform(-1, 1, (nb, len(rows))).astype(npdt)
        x = rng.uniform(-1, 1, (nb, n) if q is None else (nb, n, q)).astype(npdt)
        b = rng.uniform(-1, 1, x.shape).astype(npdt)
        r, d = _framed(npdt, [v, x, b], [x.shape, x.shape],
                       lambda a, xx, bb, ro, do: prod.residual(a, xx, bb, out=(ro, do)))
        (t,) = _framed(npdt, [v, x], [x.shape], lambda a, xx, o: prod.absMv(a, xx, out=o))
        for m in range(nb):
            wr, wd = E.residual_model(n, rows, cols, tri, v[m], x[m], b[m], npdt)
            assert _bits_equal(r[m], wr) and _bits_equal(d[m], wd), (name, dt, nb, q, m)
            assert _bits_equal(t[m], E.residual_model(n, rows, cols, tri, v[m], x[m], None, npdt)[1])
            r1, d1 = prod.residual(_dev(v[m]), _dev(x[m]), _dev(b[m]))
            assert _bits_equal(r1.cpu().numpy(), r[m]) and _bits_equal(d1.cpu().numpy(), d[m])


def test_first_use_order():
    c = R.case("arrow129")
    n, rows, cols = c["n"], c["rows"], c["cols"]
    pa, pb = (S.SymmetricPattern(rows, cols, n).product for _ in range(2))
    rng = np.random.default_rng(43)
    v, x, b = _dev(c["values"]), _dev(rng.uniform(-1, 1, (n, 3))), _dev(rng.uniform(-1, 1, (n, 3)))
    ra, da = pa.residual(v, x, b)
    ma = pa.mv(v, x)
    mb = pb.mv(v, x)
    rb, db = pb.residual(v, x, b)
    for s, t in ((ra, rb), (da, db), (ma, mb)):
        assert _bits_equal(s.cpu().numpy(), t.cpu().numpy())


# ---- maxRatio, colMax -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_max_ratio_and_col_max_bitwise(dt):
    _, npdt = DT[dt]
    sol = R.pattern("dups").solver
    rng = np.random.default_rng(44)
    for n, q in ((1, 1), (7, 3), (1023, 2), (1025, 17), (2500, 16), (3001, 1), (300, None)):
        shape = (n,) if q is None else (n, q)
        r = rng.standard_normal(shape).astype(npdt)
        d = rng.uniform(0.1, 2, shape).astype(npdt)
        r.reshape(n, -1)[rng.integers(n)] = 0
        fr = framed(npdt, [r, d])
        a, b = fr.view(0).view(shape), fr.view(1).view(shape)
        got = sol.maxRatio(a, b).cpu().numpy()
        cm = sol.colMax(a).cpu().numpy()
        fr.assert_intact(read_only=range(2))
        assert got.dtype == np.float64 and _bits_equal(got, np.asarray(E.max_ratio(r, d))), (dt, n, q)
        assert _bits_equal(cm, np.asarray(E.col_max(r))), (dt, n, q)
    for nb in (1, 2, 5):
        r = rng.standard_normal((nb, 1300, 3)).astype(npdt)
        d = rng.uniform(0.1, 2, r.shape).astype(npdt)
        got = sol.maxRatio(_dev(r), _dev(d)).cpu().numpy()
        cm = sol.colMax(_dev(r)).cpu().numpy()
        for m in range(nb):
            assert _bits_equal(got[m], E.max_ratio(r[m], d[m])) and _bits_equal(cm[m], E.col_max(r[m]))
            assert _bits_equal(sol.maxRatio(_dev(r[m]), _dev(d[m])).cpu().numpy(), got[m])
        r1 = r[:, :, 0].copy()
        assert _bits_equal(sol.maxRatio(_dev(r1), _dev(d[:, :, 0].copy()), batched=True).cpu().numpy(),
                           np.stack([E.max_ratio(r1[m], d[m, :, 0]) for m in range(nb)]))


@pytest.mark.parametrize("special", ["zero_over_zero", "nonzero_over_zero", "nan", "inf"])
def test_max_ratio_specials(special):
    sol = R.pattern("dups").solver
    r, d = np.full((1500, 2), 0.25), np.full((1500, 2), 2.0)
    at = 1207
    if special == "zero_over_zero":
        r[:, 0], d[:, 0] = 0.0, 0.0
        want0 = 0.0
    elif special == "nonzero_over_zero":
        d[at, 0] = 0.0
        want0 = np.inf
    elif special == "nan":
        d[at, 0] = np.nan
        want0 = np.nan
    else:
        r[at, 0] = np.inf
        want0 = np.inf
    got = sol.maxRatio(_dev(r), _dev(d)).cpu().numpy()
    assert _bits_equal(got, np.asarray(E.max_ratio(r, d)))
    assert got[1] == 0.125 and (np.isnan(got[0]) if np.isnan(want0) else got[0] == want0)


# ---- invNorm1 ---------------------------------------------------------------------------------------------
def _sizes_for(structure, n):
    if structure == "scalar" or n < 3:
        return None
    if structure == "wide3":
        s = [3] * (n // 3)
        return s + ([n % 3] if n % 3 else [])
    if n <= 70:
        return None
    return [1] * (n - 70) + [70]   # "arrow70": the last param 70 wide, one lump wider than 64


@functools.lru_cache(maxsize=None)
def _pattern_of(name, structure):
    A = E.matrix(name)
    n = A.shape[0]
    if structure == "arrow70":   # embedded: a well-conditioned arrowhead around the matrix
        m = n + 75
        big = np.eye(m) * 3.0
        big[:n, :n] = A
        big[-1, n:-1] = big[n:-1, -1] = 0.05
        A, n = big, m
    rows, cols, vals = E.lower_entries(A)
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=_sizes_for(structure, n))
    return pat, A, vals


_BBT = ["bbt_%d" % n for n in E.SIZES]
# the CPU matrix list in the three structures: all of it with scalar params; what fits 3-wide params; and, around
# the 70-wide last param, every matrix but the two of order 100 (whose dense restatement of order 175 adds nothing)
STRUCTURE_MATRICES = {
    "scalar": E.MATRICES,
    "wide3": ["grid6", "grid8", "bbt_12", "bbt_30", "spec_12", "spec_30"],
    "arrow70": [m for m in E.MATRICES if m not in ("bbt_100", "spec_100")],
}
# the matrices whose decoded record MUST be compared with the restatement's trace (in fp32: those of them with
# kappa_1 <= 500): their restatements are not fragile in either precision, which the test asserts again
_SPEC = ["spec_%d" % n for n in E.SIZES]
_SMALL = ["identity5", "diag7", "arrow40", E.ALT_WINS, E.PASS_LIMIT]
TRACE_COMPARED = {
    "scalar": ["n1"] + _SMALL + _BBT + _SPEC,
    "wide3": ["bbt_12", "bbt_30", "spec_12", "spec_30"],   # (the grids' symmetry makes near-ties)
    "arrow70": ["n1", "n2"] + _SMALL + _BBT[:-1] + _SPEC[:-1],
}


def _internal(pat, A):
    """A in the solver's internal order: A_int[perm[i], perm[j]] = A[i, j]"""
    inv = np.argsort(pat._to_user)
    return A[np.ix_(inv, inv)]


def _factor(pat, vals, tdt):
    L = pat.assembly.assemble(_dev(vals).to(tdt))
    pat.solver.factor(list(L) if L.dim() == 2 else L)
    return L


def _check_estimate(pat, A, got, state, npdt, scale=None, what=""):
    n = A.shape[0]
    Ai = _internal(pat, A)
    true = E.true_inv_norm1(A, scale)
    slack = n * E.kappa1(A if scale is None else A / np.outer(scale, scale)) * np.finfo(npdt).eps
    print("%s: est / true = %.6f (slack %.2e), passes %d, stop %s, alt won %s" % (
        what, got / true, slack, state["passes"], state["stopReason"], state["altWon"]))
    assert true / 3 <= got <= true * (1 + slack), what
    assert state["est"] == got
    si = None if scale is None else scale[np.argsort(pat._to_user)]
    est, trace, fragile = E.inv_norm1_model(Ai, npdt, scale=si)
    if not fragile:
        assert state["js"] == trace["js"] and state["passes"] == trace["passes"], what
        assert state["stop"] == trace["stop"], what
        if not trace.get("altTie", False):
            assert state["altWon"] == trace["altWon"], what
        assert abs(got - est) <= slack * true + 4 * np.finfo(npdt).eps * true, what
    return fragile


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("structure", ["scalar", "wide3", "arrow70"])
def test_inv_norm1_bounds_and_trace(structure, dt):
    tdt, npdt = DT[dt]
    compared, skipped = [], []
    for name in STRUCTURE_MATRICES[structure]:
        if dt == "f32" and E.kappa1(E.matrix(name)) > 500:
            skipped.append(name)
            continue
        pat, A, vals = _pattern_of(name, structure)
        L = _factor(pat, vals, tdt)
        out, st = pat.solver.invNorm1(L, return_state=True)
        state = pat.solver.readNormEstState(st)
        fragile = _check_estimate(pat, A, float(out), state, npdt, what="%s/%s/%s" % (name, structure, dt))
        if not fragile:
            compared.append(name)
    missing = [m for m in TRACE_COMPARED[structure] if m not in compared + skipped]
    assert not missing, "the traces of %s were not compared: their restatements turned fragile" % missing


def test_inv_norm1_branches():
    for name, reason in (("n2", "same column"), ("diag7", "repeated sign vector"), ("identity5", "repeated sign vector"),
                         ("n1", "order one")):
        pat, A, vals = _pattern_of(name, "scalar")
        out, st = pat.solver.invNorm1(_factor(pat, vals, torch.float64), return_state=True)
        state = pat.solver.readNormEstState(st)
        assert state["stopReason"] == reason, (name, state)
        assert abs(float(out) / E.true_inv_norm1(A) - 1) < 1e-4
        if name == "n2":   # (a tie of the main and the alt value: which one wins is not asserted)
            assert abs(state["alt"] / E.true_inv_norm1(A) - 1) < 1e-4
    for dt in ("f64", "f32"):
        tdt, npdt = DT[dt]
        # the alt branch: the alternating vector's value strictly wins and is the estimate
        pat, A, vals = _pattern_of(E.ALT_WINS, "scalar")
        out, st = pat.solver.invNorm1(_factor(pat, vals, tdt), return_state=True)
        state = pat.solver.readNormEstState(st)
        _, trace, fragile = E.inv_norm1_model(_internal(pat, A), npdt)
        assert trace["altWon"] and not fragile and not trace["altTie"]
        assert state["altWon"] and float(out) == state["alt"] == state["est"], (dt, state)
        assert abs(state["alt"] - trace["alt"]) <= 7 * E.kappa1(A) * np.finfo(npdt).eps * trace["alt"]
        assert state["alt"] > 1.2 * trace["main"]
        pat, A, vals = _pattern_of(E.PASS_LIMIT, "scalar")
        out, st = pat.solver.invNorm1(_factor(pat, vals, tdt), return_state=True)
        state = pat.solver.readNormEstState(st)
        assert state["stopReason"] == "pass limit" and state["passes"] == 5 and len(state["js"]) == 4, (dt, state)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_inv_norm1_batch_with_an_alt_member(dt):
    """a batch whose members end by three different reasons, one of them taking its value from the alt branch"""
    tdt, npdt = DT[dt]
    n = 7
    mats = [E.matrix("diag7"), E.matrix(E.ALT_WINS), E.matrix(E.PASS_LIMIT)]
    i, j = np.tril_indices(n)
    pat = S.SymmetricPattern(i, j, n)
    sol = pat.solver
    L = _factor(pat, np.stack([M[i, j] for M in mats]), tdt)
    out, st = sol.invNorm1(list(L), return_state=True)
    states = sol.readNormEstState(st)
    assert [s["stopReason"] for s in states] == ["repeated sign vector", "repeated sign vector", "pass limit"]
    assert [s["altWon"] for s in states] == [False, True, False]
    assert float(out[1]) == states[1]["alt"] == states[1]["est"]
    for m, M in enumerate(mats):
        o1, s1 = sol.invNorm1(L[m], return_state=True)
        one = sol.readNormEstState(s1)
        keys = ("js", "passes", "stop", "altWon")
        assert {k: one[k] for k in keys} == {k: states[m][k] for k in keys}, m
        assert abs(float(out[m]) - float(o1)) <= n * E.kappa1(M) * np.finfo(npdt).eps * float(o1), m
        _, trace, fragile = E.inv_norm1_model(_internal(pat, M), npdt)
        assert not fragile and {k: trace[k] for k in keys} == {k: states[m][k] for k in keys}, m


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_inv_norm1_batches(dt):
    """members that stop at different passes in one batch: each within the slack of its single call, traces equal"""
    tdt, npdt = DT[dt]
    n = 12
    rng = np.random.default_rng(45)

    def embed(M):
        A = np.diag(np.linspace(1.0, 2.0, n))
        A[:M.shape[0], :M.shape[0]] = M
        return A

    G1, G2 = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    e = 1e-3 if dt == "f64" else 0.05
    mats = [np.diag(rng.uniform(0.5, 4.0, n)), embed(E.alt_2x2(e)), G1 @ G1.T + 0.1 * n * np.eye(n),
            G2 @ G2.T + 0.1 * n * np.eye(n), embed(E.matrix("bbt_5"))]
    i, j = np.tril_indices(n)
    pat = S.SymmetricPattern(i, j, n)
    sol = pat.solver
    vals = np.stack([M[i, j] for M in mats])
    L = _factor(pat, vals, tdt)
    out, st = sol.invNorm1(list(L), return_state=True)
    states = sol.readNormEstState(st)
    out = out.cpu().numpy()
    assert out.shape == (5,) and len({s["passes"] for s in states}) > 1
    for m, M in enumerate(mats):
        o1, s1 = sol.invNorm1(L[m], return_state=True)
        one = sol.readNormEstState(s1)
        slack = n * E.kappa1(M) * np.finfo(npdt).eps
        assert abs(out[m] - float(o1)) <= slack * float(o1), m
        keys = ("js", "passes", "stop") if m == 1 else ("js", "passes", "stop", "altWon")   # (member 1: the alt tie)
        assert {k: one[k] for k in keys} == {k: states[m][k] for k in keys}, m
        true = E.true_inv_norm1(M)
        assert true / 3 <= out[m] <= true * (1 + slack), m
    ob, sb = sol.invNorm1([L[2]], return_state=True)
    assert ob.shape == (1,) and sb.shape == (1, 12)
    assert abs(float(ob[0]) - out[2]) <= n * E.kappa1(mats[2]) * np.finfo(npdt).eps * out[2]


def test_inv_norm1_work_in_a_poisoned_frame():
    pat, A, vals = _pattern_of("grid8", "scalar")
    sol, lib = pat.solver, pat.solver._lib
    L = _factor(pat, vals, torch.float64)
    need = ctypes.c_int64(0)
    assert lib.bsp_inv_norm1_work_bytes_f64(sol._h, ctypes.byref(need)) == 0
    n = sol.order()
    assert need.value == ((2 * n * 8 + 15) // 16) * 16 + 16 * max(1, (n + 1023) // 1024)
    pad = 256
    frame = torch.full((need.value + 2 * pad + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    at = (frame.data_ptr() + pad + 15) // 16 * 16 - frame.data_ptr()
    state = torch.full((14,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
    P = ctypes.c_void_p
    rc = lib.bsp_inv_norm1_f64(sol._h, P(L.data_ptr()), None, P(frame.data_ptr() + at), P(state[1:].data_ptr()),
                               P(out[1:].data_ptr()))
    assert rc == 0, lib.bsp_last_error().decode()
    torch.cuda.synchronize()
    f = frame.cpu().numpy()
    assert (f[:at] == 0x5A).all() and (f[at + need.value:] == 0x5A).all(), "written outside the workspace"
    assert state[0] == -7 and state[13] == -7 and out[0] == -7 and out[2] == -7
    true = E.true_inv_norm1(A)
    assert true / 3 <= float(out[1]) <= true * (1 + 1e-9)


@pytest.mark.parametrize("dt", ["f64"])
def test_inv_norm1_scale(dt):
    tdt, npdt = DT[dt]
    pat, A, vals = _pattern_of(E.SCALED, "scalar")
    sol = pat.solver
    L = _factor(pat, vals, tdt)
    D = np.sqrt(np.diag(A))
    Dint = pat.toInternal(_dev(D).to(tdt)).contiguous()
    out, st = sol.invNorm1(L, scale=Dint, return_state=True)
    _check_estimate(pat, A, float(out), sol.readNormEstState(st), npdt, scale=D, what="scaled30")
    raw = float(sol.invNorm1(L))
    assert raw > 1e10 * float(out)


# ---- cond_estimate, norm1 -----------------------------------------------------------------------------
def test_cond_estimate_and_norm1():
    name = "blocks"   # a pattern with params and a non-trivial permutation
    c, pat = R.case(name), R.pattern(name)
    n, rows, cols = c["n"], c["rows"], c["cols"]
    assert not np.array_equal(pat._to_user, np.arange(n))
    rng = np.random.default_rng(46)
    vals = rng.uniform(-1, 1, (3, len(rows)))
    vals[:, rows == cols] = rng.uniform(6.0, 9.0, (3, int((rows == cols).sum())))
    for scaled in (False, True):
        got1 = S.norm1(pat, _dev(vals), scaled=scaled).cpu().numpy()
        est = S.cond_estimate(pat, _dev(vals), scaled=scaled).cpu().numpy()
        assert got1.shape == (3,) and est.shape == (3,)
        for m in range(3):
            A = dense_user(n, rows, cols, vals[m])
            s = E.jacobi_scale(A) if scaled else np.ones(n)
            t = E.residual_model(n, rows, cols, "lower", vals[m], s, None, np.float64)[1]
            want = float(np.max(s * t))
            assert _bits_equal(got1[m], np.float64(want)), (scaled, m)
            assert _bits_equal(S.norm1(pat, _dev(vals[m]), scaled=scaled).cpu().numpy(), np.float64(want))
            As = A * np.outer(s, s)
            kappa = E.kappa1(As)
            slack = n * kappa * np.finfo(np.float64).eps
            print("cond_estimate scaled=%s member %d: %.4f of kappa_1 = %.3e" % (scaled, m, est[m] / kappa, kappa))
            assert kappa / 3 <= est[m] <= kappa * (1 + slack)
            one = float(S.cond_estimate(pat, _dev(vals[m]), scaled=scaled))
            assert abs(one - est[m]) <= slack * est[m]
    bad = vals[0].copy()
    bad[rows == cols] = -1.0
    est, info = S.cond_estimate(pat, _dev(bad), return_info=True)
    assert not np.isfinite(float(est))
    assert not pat.solver.readFactorStatus(info["factor_status"])["ok"]
    assert info["state"].shape == (12,)
    assert pat.solver.readNormEstState(info["state"])["stopReason"] == "non-finite"


# ---- solve_refined ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid():
    c = R.refine_case("g12_s0.1")
    pat = S.SymmetricPattern(c["rows"], c["cols"], c["n"])
    return c, pat


def test_solve_refined_defaults_unchanged():
    c, pat = _grid()
    v, b = _dev(c["values"]), _dev(c["b"])
    x = S.solve_refined(pat, v, b)
    sol = pat.solver
    L32 = pat.assembly.assemble(v.float())
    sol.factor(L32)

    def solve32(r):
        rt = pat.toInternal(r.float(), 0).t().contiguous()
        sol.solve(L32, rt, stride=c["n"], nRHS=rt.shape[0])
        return pat.fromInternal(rt.t(), 0).double()

    y = solve32(b)
    for _ in range(3):
        y = y + solve32(b - S.matvec(pat, v, y.contiguous()))
    assert _bits_equal(x.cpu().numpy(), y.contiguous().cpu().numpy())
    xi, info = S.solve_refined(pat, v, b, return_info=True)
    assert _bits_equal(xi.cpu().numpy(), x.cpu().numpy())
    assert (info["corrections"] == 3).all() and info["corrections"].dtype == torch.int64


def test_solve_refined_berr():
    c, pat = _grid()
    v, b = _dev(c["values"]), _dev(c["b"])
    x, info = S.solve_refined(pat, v, b, return_info=True)
    be = S.backward_error(pat, v, x, b)
    assert be.shape == (3,) and _bits_equal(info["berr"].cpu().numpy(), be.cpu().numpy())
    r, d = S.residual(pat, v, x, b)
    assert _bits_equal(be.cpu().numpy(), E.max_ratio(r.cpu().numpy(), d.cpu().numpy()))
    t_max = int(np.diff(R.row_terms(c["n"], c["rows"], c["cols"])[0]).max())
    bound = 4 * np.finfo(np.float64).eps * (t_max + 1)   # the model of one rounded residual
    print("berr %s, bound %.3e (t_max = %d)" % (be.cpu().numpy(), bound, t_max))
    assert float(be.max()) < bound
    assert pat.solver.readFactorStatus(info["factor_status"])["ok"]
    # a batch: member by member the single call
    vb, bb = torch.stack([v, 1.5 * v]), torch.stack([b, b])
    xb, ib = S.solve_refined(pat, vb, bb, return_info=True)
    assert ib["berr"].shape == (2, 3) and ib["corrections"].shape == (2, 3) and ib["factor_status"].shape == (2, 4)
    assert _bits_equal(xb[0].cpu().numpy(), x.cpu().numpy())
    assert _bits_equal(ib["berr"][0].cpu().numpy(), be.cpu().numpy())
    b1 = b[:, 0].contiguous()
    x1, i1 = S.solve_refined(pat, v, b1, return_info=True)
    assert i1["berr"].shape == () and _bits_equal(x1.cpu().numpy(), x[:, 0].contiguous().cpu().numpy())


def test_solve_refined_early_stop():
    c, pat = _grid()
    v, b = _dev(c["values"]), _dev(c["b"])
    x, info = S.solve_refined(pat, v, b, iters=6, tol=1e-14, return_info=True)
    print("corrections %s, berr %s" % (info["corrections"].cpu().numpy(), info["berr"].cpu().numpy()))
    assert (info["corrections"] < 6).all() and (info["berr"] <= 1e-14).all()
    assert R.rel_err(x.cpu().numpy(), c["ref"]) <= R.refine_bound("g12_s0.1")
    assert _bits_equal(S.solve_refined(pat, v, b, iters=6, tol=1e-14).cpu().numpy(), x.cpu().numpy())


def test_solve_refined_reports_no_convergence():
    rng = np.random.default_rng(2)   # (a seed whose matrix numpy's fp32 Cholesky still factors)
    n = 30
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0, 9, n)) @ Q.T
    A = (A + A.T) / 2
    b = rng.uniform(-1, 1, (n, 2))
    # the host model: numpy's fp32 Cholesky succeeds, refinement stagnates far above the tolerance
    model = R.refine_model(A, b, 4)
    host_berr = E.max_ratio(b - A @ model, np.abs(A) @ np.abs(model) + np.abs(b))
    assert np.isfinite(model).all() and host_berr.min() > 1e-12
    rows, cols, vals = E.lower_entries(A)
    pat = S.SymmetricPattern(rows, cols, n)
    x, info = S.solve_refined(pat, _dev(vals), _dev(b), iters=4, tol=1e-14, return_info=True)
    print("host berr %s, device berr %s" % (host_berr, info["berr"].cpu().numpy()))
    assert (info["corrections"] == 4).all() and (info["berr"] > 1e-14).all()


def test_solve_refined_reports_fp32_breakdown():
    n = 8
    A = np.diag(np.linspace(2.0, 3.0, n))
    A[:2, :2] = [[1.0, 1 - 1e-10], [1 - 1e-10, 1.0]]
    assert np.linalg.eigvalsh(A).min() > 0 and np.linalg.det(A[:2, :2].astype(np.float32).astype(np.float64)) == 0
    rows, cols, vals = E.lower_entries(A)
    pat = S.SymmetricPattern(rows, cols, n)
    b = _dev(np.ones(n))
    _, info = S.solve_refined(pat, _dev(vals), b, return_info=True)
    assert not pat.solver.readFactorStatus(info["factor_status"])["ok"]
    x64 = S.solve(pat, _dev(vals), b)
    assert float(S.backward_error(pat, _dev(vals), x64, b)) < 1e-14


def test_solve_refined_gradients_with_tol():
    c, pat = _grid()
    grads = []
    for kw in ({}, {"tol": 1e-14, "iters": 6}):
        v = _dev(c["values"]).requires_grad_(True)
        b = _dev(c["b"]).requires_grad_(True)
        w = _dev(np.random.default_rng(48).uniform(-1, 1, c["b"].shape))
        (S.solve_refined(pat, v, b, **kw) * w).sum().backward()
        grads.append((v.grad.cpu().numpy(), b.grad.cpu().numpy()))
    for g0, g1 in zip(*grads):
        assert np.max(np.abs(g0 - g1)) <= 1e-10 * max(1.0, np.max(np.abs(g0)))


# ---- refusals -------------------------------------------------------------------------------------------
def _refusal_setup():
    c, pat = R.case("dups"), R.pattern("dups")
    prod, sol, n, nnz = pat.product, pat.solver, c["n"], len(c["rows"])
    v = torch.rand(nnz, dtype=torch.float64, device="cuda")
    x = torch.rand(n, 2, dtype=torch.float64, device="cuda")
    b = torch.rand(n, 2, dtype=torch.float64, device="cuda")
    nan = float("nan")
    r = torch.full((n, 2), nan, dtype=torch.float64, device="cuda")
    d = torch.full((n, 2), nan, dtype=torch.float64, device="cuda")
    return c, pat, prod, sol, v, x, b, r, d


def _arr(*ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


REFUSALS = ["null_member", "null_array", "empty_batch", "q_below_one", "repeated_output", "aliased_output",
            "other_solver"]


@pytest.mark.parametrize("which", REFUSALS)
def test_residual_refusals(which):
    c, pat, prod, sol, v, x, b, r, d = _refusal_setup()
    lib, P, q2 = sol._lib, ctypes.c_void_p, ctypes.c_int64(2)
    p = lambda t: P(t.data_ptr())
    one = ctypes.c_int32(1)
    if which == "null_member":
        rc = lib.bsp_sym_product_residual_f64(sol._h, prod._h, p(v), p(x), None, q2, p(r), p(d))
        want = "right-hand side pointer of batch member 0 is NULL"
    elif which == "null_array":
        rc = lib.bsp_sym_product_residual_batched_f64(sol._h, prod._h, _arr(v), _arr(x), _arr(b), q2, None, _arr(d), one)
        want = "NULL"
    elif which == "empty_batch":
        rc = lib.bsp_sym_product_residual_batched_f64(sol._h, prod._h, _arr(v), _arr(x), _arr(b), q2, _arr(r), _arr(d),
                                                      ctypes.c_int32(0))
        want = "empty"
    elif which == "q_below_one":
        rc = lib.bsp_sym_product_abs_mv_f64(sol._h, prod._h, p(v), p(x), ctypes.c_int64(0), p(d))
        want = "q = 0"
    elif which == "repeated_output":
        rc = lib.bsp_sym_product_residual_f64(sol._h, prod._h, p(v), p(x), p(b), q2, p(r), p(r))
        want = "aliases its scale"
    elif which == "aliased_output":
        rc = lib.bsp_sym_product_residual_f64(sol._h, prod._h, p(v), p(x), p(b), q2, p(r), P(x.data_ptr() + 8))
        want = "aliases its vector"
    else:
        other = R.pattern("full")
        rc = lib.bsp_sym_product_residual_f64(other.solver._h, prod._h, p(v), p(x), p(b), q2, p(r), p(d))
        want = "another solver"
    msg = lib.bsp_last_error().decode()
    assert rc != 0 and want in msg, msg
    torch.cuda.synchronize()
    assert torch.isnan(r).all() and torch.isnan(d).all(), "a refused call launched"
    rr, dd = prod.residual(v, x, b, out=(r, d))
    wr, wd = E.residual_model(c["n"], c["rows"], c["cols"], c["triangle"], v.cpu().numpy(), x.cpu().numpy(),
                              b.cpu().numpy(), np.float64)
    assert _bits_equal(rr.cpu().numpy(), wr) and _bits_equal(dd.cpu().numpy(), wd)


@pytest.mark.parametrize("which", ["null", "empty_batch", "q_below_one", "aliased_output"])
def test_max_ratio_refusals(which):
    c, pat, prod, sol, v, x, b, r, d = _refusal_setup()
    lib, P = sol._lib, ctypes.c_void_p
    n = c["n"]
    out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    N, Q = ctypes.c_int64(n), ctypes.c_int64(2)
    if which == "null":
        rc = lib.bsp_max_ratio_f64(sol._h, P(x.data_ptr()), None, N, Q, P(out.data_ptr()))
        want = "NULL"
    elif which == "empty_batch":
        rc = lib.bsp_col_max_batched_f64(sol._h, _arr(x), N, Q, P(out.data_ptr()), ctypes.c_int32(0))
        want = "empty"
    elif which == "q_below_one":
        rc = lib.bsp_max_ratio_f64(sol._h, P(x.data_ptr()), P(b.data_ptr()), N, ctypes.c_int64(0), P(out.data_ptr()))
        want = "q = 0"
    else:
        rc = lib.bsp_max_ratio_f64(sol._h, P(x.data_ptr()), P(b.data_ptr()), N, Q, P(x.data_ptr() + 8))
        want = "aliases"
    msg = lib.bsp_last_error().decode()
    assert rc != 0 and want in msg, msg
    torch.cuda.synchronize()
    assert (out == -7).all()
    assert _bits_equal(sol.maxRatio(x, b).cpu().numpy(), E.max_ratio(x.cpu().numpy(), b.cpu().numpy()))


@pytest.mark.parametrize("which", ["null_factor", "null_work", "empty_batch", "partial_solver", "aliased_work",
                                   "aliased_output", "aliased_state"])
def test_inv_norm1_refusals(which):
    pat, A, vals = _pattern_of("grid6", "scalar")
    sol, lib, P = pat.solver, pat.solver._lib, ctypes.c_void_p
    L = _factor(pat, vals, torch.float64)
    keep = L.clone()
    need = ctypes.c_int64(0)
    assert lib.bsp_inv_norm1_work_bytes_f64(sol._h, ctypes.byref(need)) == 0
    work = torch.full((need.value // 8 + 2,), -7.0, dtype=torch.float64, device="cuda")
    wp = (work.data_ptr() + 15) // 16 * 16
    state = torch.full((12,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    args = [P(L.data_ptr()), None, P(wp), P(state.data_ptr()), P(out.data_ptr())]
    h = sol._h
    if which == "null_factor":
        args[0], want = None, "factor pointer of batch member 0 is NULL"
    elif which == "null_work":
        args[2], want = None, "workspace pointer is NULL"
    elif which == "aliased_work":
        args[2], want = P((L.data_ptr() + 15) // 16 * 16), "aliases the factor"
    elif which == "aliased_output":
        args[4], want = P(L.data_ptr() + 8), "the output aliases the factor"
    elif which == "aliased_state":
        args[3], want = P(L.data_ptr()), "the state aliases the factor"
    elif which == "partial_solver":
        from helpers import solver_random
        part, _, _ = solver_random(61, fill=0.03, elim=(0, 60), ranges=[0, 60], policy=B.AddFillForGivenElims)
        assert part.canFactorUpToSpan() < part.numSpans()
        h, want = part._h, "can only factor up to span"
        args[0] = P(torch.ones(part.dataSize(), dtype=torch.float64, device="cuda").data_ptr())
    if which == "empty_batch":
        rc = lib.bsp_inv_norm1_batched_f64(h, _arr(L), None, args[2], args[3], args[4], ctypes.c_int32(0))
        want = "empty"
    else:
        rc = lib.bsp_inv_norm1_f64(h, *args)
    msg = lib.bsp_last_error().decode()
    assert rc != 0 and want in msg, msg
    torch.cuda.synchronize()
    assert (work == -7).all() and (state == -7).all() and (out == -7).all() and torch.equal(L, keep)
    true = E.true_inv_norm1(A)
    assert true / 3 <= float(sol.invNorm1(L)) <= true * (1 + 1e-9)
