"""GPU: the entry points behind the error bounds, the conjugate gradient and the Lanczos recurrence
(bsp_sym_product_residual_* / abs_mv_*, bsp_max_ratio_* / bsp_col_max_*, bsp_inv_norm1_*, bsp_cg_*, bsp_lanczos_*)
past the chunk limit of 65535 members, and the independence of their results from what their Solver and their
entry map were asked to do before.

Past the chunk limit: a structure of order 5 with 65537 members, of which 3 are distinct and repeated, q = 2
wherever the entry takes q (so that q0 * q differs from q0 in the hand-written chunk offsets work + q0 * stride,
state + q0 * q, status + 2 * q0, coef + q0 * q * 2 * kmax, out + q0 * q, NormEstState* + q0): every member -- the
members 0, 65534, 65535 and 65536 around the boundary among them -- is bitwise the single call of its matrix;
then a batch of 2 on the same objects is.  The pointer arrays are numpy arithmetic on one base tensor.

Call history: the preconditioner plans of a map are uploaded by the first call that needs them, per kind and per
use (build, apply); the partials of maxRatio / colMax grow on demand and are shared by every call and stream of
the Solver.  Each veteran result is bitwise a fresh Solver's and the numpy restatement's.  The stream scenario
follows test_stream_and_history_of_the_solver: the hand-over of history.py, torch's own work inside the solver's
stream, a device synchronisation after every operation.  The refusals are argument checks: nothing is launched."""
import ctypes
import time

import numpy as np
import pytest
import torch

import cg_ref as R
import error_bounds_ref as E
import history as H
import iter_driver as D
import lanczos_ref as LR
from baspacho_amd import sparse as S
from buffer_edges import Frame, is_sentinel

pytestmark = pytest.mark.gpu

P, I32, I64, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
TDT = {"f64": torch.float64, "f32": torch.float32}
NPDT = {"f64": np.float64, "f32": np.float32}
BIG = 65537
AROUND = (0, 65534, 65535, 65536)
TIMES = {}


def _ibits(t):
    """a float tensor as integer words: NaNs compare like any other bits"""
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _host_same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(TDT[dt]).cuda()


def _nan(shape, tdt=torch.float64):
    return torch.full(shape, float("nan"), dtype=tdt, device="cuda")


def _sfx(t):
    return "f64" if t.dtype == torch.float64 else "f32"


def _rep(base, idx):
    """the addresses of the rows idx[m] of the contiguous tensor base [k, ...]"""
    per = base[0].numel() * base.element_size()
    return np.uint64(base.data_ptr()) + np.asarray(idx, dtype=np.uint64) * np.uint64(per)


def _each(t):
    """the addresses of the rows of the contiguous tensor t [members, ...]"""
    return _rep(t, np.arange(t.shape[0]))


def _ok(lib, rc):
    assert rc == 0, lib.bsp_last_error().decode()


def _members_are_singles(got, singles, idx, what):
    """got [members, ...] against singles [k, ...][idx], as bits, on the device; the first member that differs is
    named"""
    g = _ibits(got).reshape(got.shape[0], -1)
    s = _ibits(singles).reshape(singles.shape[0], -1)[torch.as_tensor(np.asarray(idx), device=got.device)]
    bad = (g != s).any(dim=1)
    if bool(bad.any()):
        m = int(torch.nonzero(bad)[0, 0])
        raise AssertionError((what, "member %d of %d is not the single call of its matrix" % (m, got.shape[0]),
                              "%d members differ" % int(bad.sum())))
    if got.shape[0] == BIG:
        for m in AROUND:
            assert torch.equal(g[m], s[m]), (what, m)


# ---- runs of the pieces on plain tensors ---------------------------------------------------------------------
def cg_on(sol, prod, v, b, idx, batched, kind, steps, tol=1e-6, build_prod=None):
    """a CG run through tests/iter_driver.py: member m solves with the values v[idx[m]] and the right-hand sides
    b[idx[m]] ([k, nnz], [k, n, q] device tensors); every written buffer starts as NaN.  Device tensors x [M, n, q],
    state [M, q, 12] (float64 words), status [M, 2], minv [M, elems]"""
    M, (n, q), dt = len(idx), b.shape[1:], _sfx(b)
    lib = sol._lib
    inv = 1
    if kind in (1, 2):
        info = (ctypes.c_int64 * 4)()
        _ok(lib, lib.bsp_cg_precond_info(prod._h, I32(kind), info))
        inv = max(int(info[2]), 1)
    W, Wb = D.work_bytes(sol, "cg", n, q), D.work_bytes(sol, "cg", n, 1)
    it = torch.as_tensor(np.asarray(idx), device="cuda")
    x = torch.zeros((M, n, q), dtype=b.dtype, device="cuda")
    r = b[it].clone()
    p, ap, z = (_nan((M, n, q), b.dtype) for _ in range(3))
    minv = _nan((M, inv), b.dtype)
    state, status = _nan((M, q, 12)), _nan((M, 2))
    work = torch.empty(W * M, dtype=torch.uint8, device="cuda")
    bwork = torch.empty(Wb * M, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 16 == 0 and bwork.data_ptr() % 16 == 0
    ops = {"values": _rep(v, idx), "b": _rep(b, idx), "x": _each(x), "r": _each(r), "p": _each(p), "ap": _each(ap),
           "z": None if kind is None else _each(z), "minv": _each(minv) if kind in (1, 2) else None}
    run = D.CgPieces(sol, prod, dt, n, q, M, batched, ops, work.data_ptr(), state.data_ptr(), kind=kind, tol=tol,
                     max_steps=steps, build_work=bwork.data_ptr(), status=status.data_ptr())
    if build_prod is not None:     # minv through another map; this map's first call is then the apply
        D.CgPieces(sol, build_prod, dt, n, q, M, batched, ops, work.data_ptr(), state.data_ptr(), kind=kind,
                   build_work=bwork.data_ptr(), status=status.data_ptr()).build()
        run.init()
        run.direction(-1)
        for step in range(steps):
            run.iterate(step)
    else:
        run.run()
    return {"x": x, "state": state, "status": status, "minv": minv, "_keep": (r, p, ap, z, work, bwork)}


def lz_on(sol, prod, v, v0, idx, batched, kmax, full=True, kept=True):
    """a Lanczos run through tests/iter_driver.py, as cg_on: coef [M, q, 2, kmax], state [M, q, 12], basis [M, slots,
    n, q], all NaN before"""
    M, (n, q), dt = len(idx), v0.shape[1:], _sfx(v0)
    slots = kmax if (full or kept) else min(2, kmax)
    W = D.work_bytes(sol, "lanczos", n, q, kmax)
    w = _nan((M, n, q), v0.dtype)
    basis = _nan((M, slots, n, q), v0.dtype)
    state, coef = _nan((M, q, 12)), _nan((M, q, 2, kmax))
    work = torch.empty(W * M, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 16 == 0
    ops = {"values": _rep(v, idx), "v0": _rep(v0, idx), "w": _each(w), "basis": _each(basis)}
    D.LanczosPieces(sol, prod, dt, n, q, kmax, M, batched, ops, n * q, slots, coef.data_ptr(), work.data_ptr(),
                    state.data_ptr(), full=full).run()
    return {"coef": coef, "state": state, "basis": basis, "_keep": (w, work)}


def _check_cg(res, rows, cols, n, sizes, vals, b, idx, dt, kind, steps, tol=1e-6):
    """against cg_ref.entries_model, member by member"""
    x = res["x"].cpu().numpy()
    state = res["state"].cpu().numpy().view(np.int64)
    status = res["status"].cpu().numpy().view(np.int64)
    precond = {None: None, 1: "jacobi", 2: "block_jacobi"}[kind]
    for m, k in enumerate(idx):
        want, st, stat = R.entries_model(n, rows, cols, vals[k].astype(NPDT[dt]), b[k].astype(NPDT[dt]), NPDT[dt], precond,
                                         param_sizes=sizes, tol=tol, max_steps=steps)
        assert _host_same(x[m], want), ("x", m)
        for j in range(b.shape[2]):
            np.testing.assert_array_equal(state[m, j], R.record_words(st, j), err_msg="member %d column %d" % (m, j))
        if kind is not None:
            np.testing.assert_array_equal(status[m], stat)


def _check_lz(res, rows, cols, n, vals, v0, idx, dt, kmax, full=True):
    coef = res["coef"].cpu().numpy()
    state = res["state"].cpu().numpy().view(np.int64)
    basis = res["basis"].cpu().numpy()
    for m, k in enumerate(idx):
        want, st, V = LR.entries_model(n, rows, cols, vals[k].astype(NPDT[dt]), v0[k].astype(NPDT[dt]), NPDT[dt], kmax,
                                       reorth="full" if full else None)
        for c in range(v0.shape[2]):
            np.testing.assert_array_equal(state[m, c], LR.record_words(st, c), err_msg="member %d column %d" % (m, c))
            s = int(st["steps"][c])
            assert _host_same(coef[m, c, :, :s], want[c, :, :s]), ("alpha, beta", m, c)
            assert np.isnan(coef[m, c, :, s:]).all(), ("a coefficient beyond the steps done", m, c)
            if basis.shape[1] == kmax:
                assert _host_same(basis[m, :s, :, c], V[:s, :, c]), ("basis", m, c)


# ---- past the chunk limit ----------------------------------------------------------------------------------------
def _tiny():
    """order 5 over params of 2, 1 and 2 scalars: a tridiagonal matrix with one diagonal entry given twice; three
    sets of values, right-hand sides / start vectors [3, 5, 2]"""
    n = 5
    rows, cols, _ = R.tridiagonal(n)
    rows, cols = np.concatenate([rows, [0]]), np.concatenate([cols, [0]])
    rng = np.random.default_rng(65537)
    vals = np.stack([np.concatenate([3.0 + rng.uniform(0, 1, n), -1.0 + rng.uniform(-0.1, 0.1, n - 1), [0.3]])
                     for _ in range(3)])
    b = rng.uniform(-1, 1, (3, n, 2))
    sizes = [2, 1, 2]
    return n, rows, cols, vals, b, sizes, S.SymmetricPattern(rows, cols, n, param_sizes=sizes)


IDX = np.arange(BIG) % 3


def _timed(name, t0):
    torch.cuda.synchronize()
    TIMES[name] = time.perf_counter() - t0
    print("batch of %d, %s: %.2f s" % (BIG, name, TIMES[name]))


def test_residual_and_abs_mv_past_the_chunk_limit_then_a_batch_of_two():
    n, rows, cols, vals, b, sizes, pat = _tiny()
    sol, prod, lib, q = pat.solver, pat.product, pat.solver._lib, 2
    v3, x3, b3 = _dev(vals, "f32"), _dev(b[::-1].copy(), "f32"), _dev(b, "f32")
    singles = [torch.stack(t) for t in zip(*[prod.residual(v3[k], x3[k], b3[k]) + (prod.absMv(v3[k], x3[k]),)
                                             for k in range(3)])]
    t0 = time.perf_counter()
    r, d, t = (_nan((BIG, n, q), torch.float32) for _ in range(3))
    vp, xp, bp = _rep(v3, IDX), _rep(x3, IDX), _rep(b3, IDX)
    a = lambda arr: arr.ctypes.data_as(P)
    _ok(lib, lib.bsp_sym_product_residual_batched_f32(sol._h, prod._h, a(vp), a(xp), a(bp), I64(q), a(_each(r)),
                                                      a(_each(d)), I32(BIG)))
    _ok(lib, lib.bsp_sym_product_abs_mv_batched_f32(sol._h, prod._h, a(vp), a(xp), I64(q), a(_each(t)), I32(BIG)))
    for got, one, what in zip((r, d, t), singles, ("residual r", "residual d", "absMv")):
        _members_are_singles(got, one, IDX, what)
    _timed("residual + absMv", t0)
    r2, d2 = prod.residual(v3[:2].contiguous(), x3[:2].contiguous(), b3[:2].contiguous())
    t2 = prod.absMv(v3[:2].contiguous(), x3[:2].contiguous())
    for got, one, what in zip((r2, d2, t2), singles, ("residual r", "residual d", "absMv")):
        _members_are_singles(got, one, [0, 1], what + ", batch of 2 after %d" % BIG)


def test_max_ratio_and_col_max_past_the_chunk_limit_then_a_batch_of_two():
    n, rows, cols, vals, b, sizes, pat = _tiny()
    sol, lib, q = pat.solver, pat.solver._lib, 2
    rng = np.random.default_rng(3)
    r3, d3 = _dev(b, "f32"), _dev(rng.uniform(0.1, 2, b.shape), "f32")
    singles = [torch.stack([sol.maxRatio(r3[k], d3[k]) for k in range(3)]),
               torch.stack([sol.colMax(r3[k]) for k in range(3)])]
    for k in range(3):
        assert _host_same(singles[0][k].cpu().numpy(), np.asarray(E.max_ratio(r3[k].cpu().numpy(), d3[k].cpu().numpy())))
        assert _host_same(singles[1][k].cpu().numpy(), np.asarray(E.col_max(r3[k].cpu().numpy())))
    assert len({singles[0][k].cpu().numpy().tobytes() for k in range(3)}) == 3
    t0 = time.perf_counter()
    a = lambda arr: arr.ctypes.data_as(P)
    for M, idx in ((BIG, IDX), (2, np.array([0, 1]))):
        ratio, cmax = _nan((M, q)), _nan((M, q))
        _ok(lib, lib.bsp_max_ratio_batched_f32(sol._h, a(_rep(r3, idx)), a(_rep(d3, idx)), I64(n), I64(q),
                                               P(ratio.data_ptr()), I32(M)))
        _ok(lib, lib.bsp_col_max_batched_f32(sol._h, a(_rep(r3, idx)), I64(n), I64(q), P(cmax.data_ptr()), I32(M)))
        _members_are_singles(ratio, singles[0], idx, "maxRatio, batch of %d" % M)
        _members_are_singles(cmax, singles[1], idx, "colMax, batch of %d" % M)
        if M == BIG:
            _timed("maxRatio + colMax", t0)


def test_inv_norm1_past_the_chunk_limit_then_a_batch_of_two():
    n, rows, cols, vals, b, sizes, pat = _tiny()
    sol, lib = pat.solver, pat.solver._lib
    L3 = pat.assembly.assemble(_dev(vals, "f32"))
    sol.factor(list(L3))
    ones = [sol.invNorm1(L3[k], return_state=True) for k in range(3)]
    est1, st1 = torch.stack([o[0] for o in ones]), torch.stack([o[1] for o in ones])
    for k in range(3):
        A = np.zeros((n, n))
        np.add.at(A, (rows, cols), vals[k])
        A = A + np.tril(A, -1).T
        true = E.true_inv_norm1(A)
        assert true / 3 <= float(est1[k]) <= true * (1 + n * E.kappa1(A) * np.finfo(np.float32).eps)
    need = ctypes.c_int64(0)
    _ok(lib, lib.bsp_inv_norm1_work_bytes_f32(sol._h, ctypes.byref(need)))
    t0 = time.perf_counter()
    for M, idx in ((BIG, IDX), (2, np.array([0, 1]))):
        work = torch.empty(need.value * M, dtype=torch.uint8, device="cuda")
        state = torch.full((M, 12), -7, dtype=torch.int64, device="cuda")
        out = _nan((M,))
        lp = _rep(L3, idx)
        _ok(lib, lib.bsp_inv_norm1_batched_f32(sol._h, lp.ctypes.data_as(P), None, P(work.data_ptr()),
                                               P(state.data_ptr()), P(out.data_ptr()), I32(M)))
        _members_are_singles(out.unsqueeze(1), est1.unsqueeze(1), idx, "the estimate, batch of %d" % M)
        _members_are_singles(state.view(torch.float64), st1.view(torch.float64), idx, "the 12 state words, batch of %d" % M)
        if M == BIG:
            _timed("invNorm1", t0)


@pytest.mark.parametrize("kind", [1, 2], ids=["jacobi", "block_jacobi"])
def test_cg_past_the_chunk_limit_then_a_batch_of_two(kind):
    n, rows, cols, vals, b, sizes, pat = _tiny()
    sol, prod = pat.solver, pat.product
    v3, b3 = _dev(vals, "f32"), _dev(b, "f32")
    ones = [cg_on(sol, prod, v3, b3, [k], False, kind, 4) for k in range(3)]
    _check_cg({k: torch.cat([o[k] for o in ones]) for k in ("x", "state", "status")}, rows, cols, n, sizes, vals, b,
              [0, 1, 2], "f32", kind, 4)
    t0 = time.perf_counter()
    for M, idx in ((BIG, IDX), (2, np.array([0, 1]))):
        got = cg_on(sol, prod, v3, b3, idx, True, kind, 4)
        for k in ("x", "state", "status", "minv"):
            _members_are_singles(got[k], torch.cat([o[k] for o in ones]), idx, "cg %s, batch of %d" % (k, M))
        if M == BIG:
            _timed("cg kind %d" % kind, t0)


def test_lanczos_past_the_chunk_limit_then_a_batch_of_two():
    n, rows, cols, vals, b, sizes, pat = _tiny()
    sol, prod = pat.solver, pat.product
    v3, z3 = _dev(vals, "f32"), _dev(b, "f32")
    ones = [lz_on(sol, prod, v3, z3, [k], False, 3) for k in range(3)]
    _check_lz({k: torch.cat([o[k] for o in ones]) for k in ("coef", "state", "basis")}, rows, cols, n, vals, b, [0, 1, 2],
              "f32", 3)
    t0 = time.perf_counter()
    for M, idx in ((BIG, IDX), (2, np.array([0, 1]))):
        got = lz_on(sol, prod, v3, z3, idx, True, 3)
        for k in ("coef", "state", "basis"):
            _members_are_singles(got[k], torch.cat([o[k] for o in ones]), idx, "lanczos %s, batch of %d" % (k, M))
        if M == BIG:
            _timed("lanczos", t0)


# ---- call history of the solver-owned state --------------------------------------------------------------------
class Scene:
    """the block-sparse matrix of the CG and Lanczos suites (order 40, params of 1 to 9 scalars), two sets of
    values, right-hand sides [2, n, 3] with one zero column; fresh() gives a new pattern on a new Solver"""

    def __init__(self):
        self.rows, self.cols, values, self.A, self.n = R.bs_case()
        rng = np.random.default_rng(12)
        self.vals = np.stack([values, values * rng.uniform(0.999, 1.001, len(values))])
        self.b = rng.uniform(-1, 1, (2, self.n, 3))
        self.b[1, :, 2] = 0.0
        self.sizes = R.BS_SIZES
        self._fresh = {}

    def fresh(self):
        return S.SymmetricPattern(self.rows, self.cols, self.n, param_sizes=self.sizes)

    def call(self, pat, what, dt, prod=None):
        """one operation on the pattern's Solver and map (or the map `prod` of that Solver): host results"""
        sol, prod = pat.solver, prod or pat.product
        v, b = _dev(self.vals, dt), _dev(self.b, dt)
        if what in ("cg1", "cg2", "cg0"):
            kind = {"cg1": 1, "cg2": 2, "cg0": None}[what]
            res = cg_on(sol, prod, v, b, [0, 1], True, kind, 5)
        elif what in ("apply1", "apply2"):
            other = sol.symProduct(self.rows, self.cols)    # the same entry list, another map
            res = cg_on(sol, prod, v, b, [0, 1], True, int(what[-1]), 5, build_prod=other)
        elif what == "lanczos":
            res = lz_on(sol, prod, v, b, [0, 1], True, 5)
        elif what == "mv":
            res = {"mv": prod.mv(v, b)}
        elif what == "residual":
            r, d = prod.residual(v, b.flip(0).contiguous(), b)
            res = {"r": r, "d": d, "absMv": prod.absMv(v, b)}
        elif what == "colMax":
            res = {"colMax": sol.colMax(b), "maxRatio": sol.maxRatio(b, b.abs() + 0.5)}
        else:
            raise KeyError(what)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in res.items() if not k.startswith("_")}

    def fresh_result(self, what, dt):
        """the operation as the only one of a new Solver, checked against its restatement, kept"""
        key = (what, dt)
        if key not in self._fresh:
            got = self.call(self.fresh(), "cg" + what[-1] if what.startswith("apply") else what, dt)
            self.restated(what, dt, got)
            self._fresh[key] = got
        return self._fresh[key]

    def restated(self, what, dt, got):
        npdt, idx = NPDT[dt], [0, 1]
        dev = {k: torch.from_numpy(a) for k, a in got.items()}
        if what.startswith(("cg", "apply")):
            kind = {"0": None, "1": 1, "2": 2}[what[-1]]
            _check_cg(dev, self.rows, self.cols, self.n, self.sizes, self.vals, self.b, idx, dt, kind, 5)
        elif what == "lanczos":
            _check_lz(dev, self.rows, self.cols, self.n, self.vals, self.b, idx, dt, 5)
        elif what == "mv":
            prod = R.Product(self.n, self.rows, self.cols)
            for m in idx:
                assert _host_same(got["mv"][m], prod.mv(self.vals[m].astype(npdt), self.b[m].astype(npdt), npdt)), m
        elif what == "residual":
            for m in idx:
                wr, wd = E.residual_model(self.n, self.rows, self.cols, "lower", self.vals[m].astype(npdt),
                                          self.b[1 - m].astype(npdt), self.b[m].astype(npdt), npdt)
                assert _host_same(got["r"][m], wr) and _host_same(got["d"][m], wd), m
        elif what == "colMax":
            bb = self.b.astype(npdt)
            for m in idx:
                assert _host_same(got["colMax"][m], np.asarray(E.col_max(bb[m])))
                assert _host_same(got["maxRatio"][m], np.asarray(E.max_ratio(bb[m], np.abs(bb[m]) + npdt(0.5))))

    def veteran_is_fresh(self, pat, what, dt, tag, prod=None):
        got = self.call(pat, what, dt, prod=prod)
        want = self.fresh_result(what, dt)
        assert set(got) == set(want)
        for k in got:
            assert _host_same(got[k], want[k]), (tag, what, dt, k, "the veteran is not bitwise the fresh Solver")
        self.restated(what, dt, got)


_SCENE = []


def _scene():
    if not _SCENE:
        _SCENE.append(Scene())
    return _SCENE[0]


ORDERS = {
    "block_jacobi-first": [("cg2", "f64"), ("cg1", "f64"), ("mv", "f64"), ("residual", "f64")],
    "jacobi-first": [("cg1", "f64"), ("cg2", "f64"), ("cg1", "f32")],
    "f32-before-f64": [("cg2", "f32"), ("cg2", "f64"), ("cg1", "f32"), ("cg1", "f64"), ("lanczos", "f32"), ("lanczos", "f64")],
    "product-first": [("mv", "f64"), ("residual", "f64"), ("cg1", "f64"), ("cg2", "f64"), ("lanczos", "f64")],
    "residual-first": [("residual", "f32"), ("cg2", "f32"), ("mv", "f32"), ("cg1", "f32")],
    "apply-jacobi-first": [("apply1", "f64"), ("cg2", "f64"), ("cg1", "f64")],
    "apply-block_jacobi-first": [("apply2", "f32"), ("cg1", "f32"), ("apply2", "f64"), ("mv", "f64")],
}


@pytest.mark.parametrize("order", list(ORDERS))
def test_first_use_order_of_the_preconditioner_plans(order):
    """every sequence starts on a new map of a new Solver; each call is bitwise the same call as the only one of
    a fresh Solver, and bitwise its restatement.  apply1 / apply2: the minv is built through another map of the
    same entry list, so that the apply is the first call this map's plan of that kind sees"""
    sc = _scene()
    pat = sc.fresh()
    for k, (what, dt) in enumerate(ORDERS[order]):
        sc.veteran_is_fresh(pat, what, dt, "%s, call %d" % (order, k))


@pytest.mark.parametrize("interleaved", [False, True], ids=["colMax", "colMax+maxRatio"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_shared_reduction_scratch_grows_between_queued_calls(dt, interleaved):
    """colMax at (batch 2, q 1, n 255), then, with nothing waited for in between, at (batch 5, q 3, n 2049), which
    makes the partials kept with the Solver grow, then the first call again: all bitwise the numpy statement and a
    fresh Solver's"""
    sc = _scene()
    rng = np.random.default_rng(13)
    small, large = rng.standard_normal((2, 255, 1)), rng.standard_normal((5, 2049, 3))
    ds, dl = rng.uniform(0.1, 2, small.shape), rng.uniform(0.1, 2, large.shape)
    a1, a2, d1, d2 = (_dev(x, dt) for x in (small, large, ds, dl))
    torch.cuda.synchronize()
    sol = sc.fresh().solver
    outs = []
    for a, d in ((a1, d1), (a2, d2), (a1, d1)):        # queued: the results are read after the last call only
        outs.append((sol.colMax(a), sol.maxRatio(a, d) if interleaved else None))
    torch.cuda.synchronize()
    for (cm, mr), (a, d) in zip(outs, ((a1, d1), (a2, d2), (a1, d1))):
        fresh = sc.fresh().solver
        ah, dh = a.cpu().numpy(), d.cpu().numpy()
        assert _host_same(cm.cpu().numpy(), fresh.colMax(a).cpu().numpy()), (tuple(a.shape), "colMax against fresh")
        for m in range(a.shape[0]):
            assert _host_same(cm[m].cpu().numpy(), np.asarray(E.col_max(ah[m]))), (tuple(a.shape), m)
            if interleaved:
                assert _host_same(mr[m].cpu().numpy(), np.asarray(E.max_ratio(ah[m], dh[m]))), (tuple(a.shape), m)
        if interleaved:
            assert _host_same(mr.cpu().numpy(), fresh.maxRatio(a, d).cpu().numpy()), (tuple(a.shape), "maxRatio against fresh")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_stream_changes(dt):
    """colMax / maxRatio, a CG run and a Lanczos run on the default stream, on a second stream handed over through
    an event, and on the default stream again (history._second_stream / _default_stream; torch's own work inside
    the solver's stream; the device waited for after every operation)"""
    sc = _scene()
    pat = sc.fresh()
    sol = pat.solver
    calls = ("colMax", "cg2", "lanczos", "cg1")
    for what in calls:          # the fresh Solvers run on the default stream, before any stream is handed over
        sc.fresh_result(what, dt)
    try:
        for phase, switch in (("default", None), ("second", H._second_stream), ("default again", H._default_stream)):
            if switch is not None:
                switch(sol)
            for what in calls:
                with H.TorchHooks.scope(sol):
                    sc.veteran_is_fresh(pat, what, dt, "stream: " + phase)
                torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        sol.setStream(None)


def _refused(lib, rc, want):
    msg = lib.bsp_last_error().decode()
    assert rc != 0 and want in msg, (rc, msg)
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", ["cg", "lanczos", "inv_norm1", "max_ratio"])
def test_after_a_refusal(family):
    """refused calls (a misaligned work area, an aliased output, a count out of range) write nothing -- their
    operands lie in frames of sentinels -- and the next valid call on the same Solver and map is bitwise the
    fresh one"""
    sc = _scene()
    pat = sc.fresh()
    sol, prod, lib = pat.solver, pat.product, pat.solver._lib
    n, q = sc.n, 3
    nq = n * q
    vec = Frame([nq, nq, nq, nq], np.float64, guard=256)         # b / v0 / r, x / w, r / basis slot, p
    for k in range(4):
        vec.fill(k, np.random.default_rng(k).uniform(-1, 1, nq))
    words = Frame([q * 12, q * 2 * 5, 1], np.float64, guard=256)  # state, coef, out
    addr = lambda fr, k: fr.view(k).data_ptr()
    N, Q = I64(n), I64(q)
    if family == "cg":
        W = D.work_bytes(sol, "cg", n, q)
        work = Frame([W // 8 + 2], np.float64, guard=256, align_bytes=16)
        vec.seal(), words.seal(), work.seal()
        wp = addr(work, 0)
        _refused(lib, lib.bsp_cg_init_f64(sol._h, N, Q, P(addr(vec, 0)), P(addr(vec, 1)), P(addr(vec, 2)), F64(1e-8), I64(5),
                                          I32(1), P(wp + 8), P(addr(words, 0))), "not 16-byte aligned")
        _refused(lib, lib.bsp_cg_update_f64(sol._h, N, Q, P(addr(vec, 3)), P(addr(vec, 0)), P(addr(vec, 3) + 8),
                                            P(addr(vec, 2)), I32(1), P(wp), P(addr(words, 0))), "aliases")
        _refused(lib, lib.bsp_cg_alpha_f64(sol._h, N, I64(0), P(addr(vec, 3)), P(addr(vec, 0)), P(wp), P(addr(words, 0))),
                 "q = 0")
        after = ("cg2", "cg1", "cg0")
    elif family == "lanczos":
        W = D.work_bytes(sol, "lanczos", n, q, 5)
        work = Frame([W // 8 + 2], np.float64, guard=256, align_bytes=16)
        vec.seal(), words.seal(), work.seal()
        wp = addr(work, 0)
        head = (sol._h, N, Q, I64(5))
        _refused(lib, lib.bsp_lanczos_init_f64(*head, P(addr(vec, 0)), P(addr(vec, 2)), I64(nq), I64(1), I64(0), F64(1e-9),
                                               P(wp + 8), P(addr(words, 0))), "not 16-byte aligned")
        _refused(lib, lib.bsp_lanczos_project_f64(*head, P(addr(vec, 1)), P(addr(vec, 2)), I64(nq), I64(1), I64(2), P(wp),
                                                  P(addr(words, 0))), "count = 2")
        _refused(lib, lib.bsp_lanczos_normalize_f64(*head, P(addr(vec, 1)), P(addr(vec, 2)), I64(nq), I64(1), I64(1), P(wp),
                                                    P(addr(words, 0))), "slot 1 is outside")
        after = ("lanczos",)
    elif family == "inv_norm1":
        L = pat.assembly.assemble(_dev(sc.vals[0], "f64"))
        sol.factor(L)
        keep = L.clone()
        need = ctypes.c_int64(0)
        _ok(lib, lib.bsp_inv_norm1_work_bytes_f64(sol._h, ctypes.byref(need)))
        work = Frame([need.value // 8 + 2], np.float64, guard=256, align_bytes=16)
        vec.seal(), words.seal(), work.seal()
        wp = addr(work, 0)
        _refused(lib, lib.bsp_inv_norm1_f64(sol._h, P(L.data_ptr()), None, P(wp + 8), P(addr(words, 0)), P(addr(words, 2))),
                 "not 16-byte aligned")
        _refused(lib, lib.bsp_inv_norm1_f64(sol._h, P(L.data_ptr()), None, P(wp), P(addr(words, 0)), P(addr(words, 0) + 8)),
                 "the output aliases the state")
        _refused(lib, lib.bsp_inv_norm1_batched_f64(sol._h, (ctypes.c_void_p * 1)(L.data_ptr()), None, P(wp),
                                                    P(addr(words, 0)), P(addr(words, 2)), I32(0)), "empty")
        assert torch.equal(L, keep)
        fresh = sc.fresh()
        Lf = fresh.assembly.assemble(_dev(sc.vals[0], "f64"))
        fresh.solver.factor(Lf)
        e1, s1 = sol.invNorm1(L, return_state=True)
        e2, s2 = fresh.solver.invNorm1(Lf, return_state=True)
        assert torch.equal(_ibits(e1), _ibits(e2)) and torch.equal(s1, s2), "invNorm1 after a refusal is not the fresh one"
        true = E.true_inv_norm1(sc.A)
        assert true / 3 <= float(e1) <= true * (1 + n * E.kappa1(sc.A) * np.finfo(np.float64).eps)
        after = ("colMax",)
    else:
        work = Frame([2], np.float64, guard=256, align_bytes=16)
        vec.seal(), words.seal(), work.seal()
        _refused(lib, lib.bsp_max_ratio_f64(sol._h, P(addr(vec, 0)), P(addr(vec, 1)), N, Q, P(addr(vec, 1) + 8)), "aliases")
        _refused(lib, lib.bsp_col_max_f64(sol._h, P(addr(vec, 0)), N, I64(0), P(addr(words, 2))), "q = 0")
        _refused(lib, lib.bsp_max_ratio_f64(sol._h, P(addr(vec, 0)), None, N, Q, P(addr(words, 2))), "NULL")
        after = ("colMax", "cg2")
    for fr, name in ((vec, "vectors"), (words, "records"), (work, "work")):
        fr.assert_intact(read_only=range(len(fr)), what="a refused %s call wrote to the %s" % (family, name))
    assert is_sentinel(words.host(0)).all() and is_sentinel(words.host(1)).all()
    for what in after:
        sc.veteran_is_fresh(pat, what, "f64", "after a refused %s call" % family)
