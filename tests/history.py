"""History independence of a Solver: the harness of tests/test_history_gpu.py and tests/test_history_cpu.py.

A Solver keeps plans, schedules, scratch that only grows, a ring of pointer slots and lazily built
extension state between calls (csrc/hip_context.h).  run_history() runs a sequence of operations on one
long-lived "veteran" Solver and each of them on a "fresh" Solver that is used once; both must pass the
operation's existing high-precision check at its existing tolerance, inputs documented as read-only must
come back bitwise unchanged, and for the operations that the suite already holds to bitwise
reproducibility the veteran's result must be bitwise the fresh one's (after two fresh Solvers agreed,
so that a mismatch can only come from history).

An operation (Op) is a name, a family, build(solver, dtype, batch, nrhs, seed) -> inputs,
run(solver, inputs) -> outputs and check(inputs, outputs).  VOCABULARY is the list for the real
Solver; random_history() draws a walk from the names of a vocabulary alone, so the coverage of a set
of seeds is computed without a GPU and a fake vocabulary of the same names gets the same walks.

Nothing here touches the GPU at import; the real operations do when they are built or run."""
import collections
import contextlib

import numpy as np

import known_factor as KF
from autograd_ref import element_coords, pattern_grad_ref
from chol_adjoint_ref import dense_factor, dense_grad, lbar_random, rel_error
from factor_status_ref import damp as damp_ref
from factor_status_ref import scan as scan_ref
from partial_adjoint_ref import bar_of, oracle as partial_oracle, splits
from selinv_adjoint_ref import dense_lbar, grad_random
from selinv_ref import corr_error, dense_reference, stored_entries

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = (F64, F32)
BATCHES = (1, 1, 2, 5, 17)
NRHS = (1, 3, 8, 16, 17)

# the bounds of the tests that own each operation, unchanged
SELINV_TOL = {F64: 2.5e-14, F32: 1e-5}          # test_selinv_gpu.py (correlation units)
INVBLK_TOL = {F64: 1.33e-14, F32: 7.7e-6}       # test_inverse_blocks_gpu.py (correlation units)
REF_RES = 1e-14
ADJOINT_TOL = {F64: 1e-10, F32: 1e-4}           # test_chol_adjoint_gpu.py, test_selinv_adjoint_gpu.py, test_partial_adjoint_gpu.py
LOGDET_TOL = {F64: 1e-12, F32: 1e-5}            # test_autograd_gpu.py
PATTERN_GRAD_TOL = {F64: 1e-13, F32: 1e-5}      # test_autograd_gpu.py (times max |want| times nRHS)
PATTERN_OUTER_TOL = {F64: 1e-14, F32: 1e-6}     # test_chol_adjoint_gpu.py

REQUIRED_FAMILIES = ("factor", "solve", "partial_solve", "addmv", "selinv", "status", "pattern", "adjoint", "reach")

Step = collections.namedtuple("Step", "op dtype batch nrhs seed")


class Op:
    """bitwise: keys of the outputs that two runs on equal inputs must give bitwise equal (the operations
    for which the suite asserts torch.equal / bitwise_equal of two runs); control: run() changes a mode of
    the solver (it is replayed on every fresh solver of the later steps); uses_batch / uses_nrhs: whether
    the operation's work depends on them (for the coverage conditions)"""

    def __init__(self, name, family, build, run, check, bitwise=(), control=False, uses_batch=False,
                 uses_nrhs=False):
        self.name, self.family = name, family
        self.build, self.run, self.check = build, run, check
        self.bitwise, self.control = tuple(bitwise), control
        self.uses_batch, self.uses_nrhs = uses_batch, uses_nrhs

    def __repr__(self):
        return self.name


def describe(steps):
    """one line per step; eval-free: history.parse(VOCABULARY, lines) gives the steps back"""
    return ["%s:%s:b%d:r%d:s%d" % (s.op.name, np.dtype(s.dtype).name, s.batch, s.nrhs, s.seed) for s in steps]


def parse(vocabulary, lines):
    by_name = {op.name: op for op in vocabulary}
    out = []
    for ln in lines:
        name, dt, b, r, s = ln.split(":")
        out.append(Step(by_name[name], np.dtype(dt), int(b[1:]), int(r[1:]), int(s[1:])))
    return out


def random_history(seed, length, vocabulary):
    """a walk of `length` steps: the dtype switches at every other step on average, batch and nRHS are drawn
    anew for every step; about one step in eight is a control operation (forcePerOp, collectOpStats,
    setStream), and one family in ten a call that is refused.  Depends on the names, families and order of
    `vocabulary` only"""
    rng = np.random.default_rng(seed)
    ctrl = [op for op in vocabulary if op.control]
    families = collections.OrderedDict()
    for op in vocabulary:
        if not op.control:
            families.setdefault(op.family, []).append(op)
    names = list(families)
    steps, dt, last = [], int(rng.integers(2)), None
    for _ in range(length):
        if ctrl and rng.random() < 0.12:
            op = ctrl[int(rng.integers(len(ctrl)))]
        else:
            # a family other than the last one (every ordered pair of families is then equally likely), then
            # one of its operations
            pick = [f for f in names if f != last]
            last = pick[int(rng.integers(len(pick)))]
            op = families[last][int(rng.integers(len(families[last])))]
        if rng.random() < 0.5:
            dt = 1 - dt
        steps.append(Step(op, DTYPES[dt], int(BATCHES[int(rng.integers(len(BATCHES)))]),
                          int(NRHS[int(rng.integers(len(NRHS)))]), int(rng.integers(1, 1000000))))
    return steps


def coverage(walks):
    """what a set of walks covers, from the steps alone: the ordered pairs (family, next family) of
    consecutive non-control steps, the dtype switches, and whether the batch / nRHS of a step that uses it is
    smaller than that of the last step that used it"""
    pairs, switches = set(), set()
    batch_down = nrhs_down = False
    for steps in walks:
        last = last_b = last_r = None
        for s in steps:
            if s.op.control:
                continue
            if last is not None:
                pairs.add((last.op.family, s.op.family))
                if last.dtype != s.dtype:
                    switches.add((np.dtype(last.dtype).name, np.dtype(s.dtype).name))
            if s.op.uses_batch:
                batch_down |= last_b is not None and s.batch < last_b
                last_b = s.batch
            if s.op.uses_nrhs:
                nrhs_down |= last_r is not None and s.nrhs < last_r
                last_r = s.nrhs
            last = s
    return {"pairs": pairs, "switches": switches, "batch_down": batch_down, "nrhs_down": nrhs_down}


def missing_coverage(walks, families=REQUIRED_FAMILIES):
    """the coverage conditions that `walks` (of one structure) miss; empty when all hold"""
    c = coverage(walks)
    out = [("pair", a, b) for a in families for b in families if a != b and (a, b) not in c["pairs"]]
    out += [("switch",) + sw for sw in (("float64", "float32"), ("float32", "float64")) if sw not in c["switches"]]
    out += [(k,) for k in ("batch_down", "nrhs_down") if not c[k]]
    return out


# ---- the runner --------------------------------------------------------------------------------------

class TorchHooks:
    """how the runner waits for a solver's work and which stream torch itself uses beside it.  The runner
    waits for the device after every operation (it reads the results on the host), so no two operations of a
    history are in flight together: the sequences that must stay queued (the pointer ring's wrap and growth)
    are written out by hand in tests/test_history_gpu.py"""

    @staticmethod
    def sync(solver):
        import torch
        torch.cuda.synchronize()

    @staticmethod
    def scope(solver):
        import torch
        st = getattr(solver, "_stream", None)
        return torch.cuda.stream(st) if st is not None and not isinstance(st, int) else contextlib.nullcontext()

    @staticmethod
    def to_host(x):
        import torch
        if isinstance(x, torch.Tensor):
            return x.detach().cpu().numpy()
        if isinstance(x, (list, tuple)):
            return [TorchHooks.to_host(v) for v in x]
        if isinstance(x, dict):
            return {k: TorchHooks.to_host(v) for k, v in x.items()}
        return x


class HostHooks:
    """for solvers that live on the host (tests/test_history_cpu.py)"""
    sync = staticmethod(lambda solver: None)
    scope = staticmethod(lambda solver: contextlib.nullcontext())
    to_host = staticmethod(lambda x: x)


class HistoryError(AssertionError):
    pass


def _same_bits(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _run_one(solver, step, inputs, hooks):
    """outputs on the host; the inputs documented as read-only (outputs["_readonly"]: (name, buffer after
    the call, host original)) are compared here"""
    with hooks.scope(solver):
        out = step.op.run(solver, inputs)
    hooks.sync(solver)
    out = hooks.to_host(out) if out is not None else {}
    for name, after, before in out.pop("_readonly", []):
        assert _same_bits(after, before), "the read-only input %s was written" % name
    return out


def run_history(make_solver, steps, tag="", hooks=TorchHooks, compare=True, report=None):
    """the steps in order on one veteran solver, each of them on a fresh one; see the module docstring.
    compare=False leaves out the bitwise veteran / fresh comparison (to show that it is what catches a
    leak that stays inside the tolerances).  report: a dict that collects, per family, the worst
    error / tolerance of veteran and fresh (from the ratios that the checks return)."""
    steps = list(steps)
    veteran = make_solver()
    modes = collections.OrderedDict()  # control op name -> (step, inputs), replayed on fresh solvers

    def fail(k, who, e):
        lines = describe(steps[:k + 1])
        raise HistoryError("history %s: %s failed at step %d (%s): %s: %s\nsteps so far: %r"
                           % (tag, who, k, lines[-1], type(e).__name__, e, lines)) from e

    for k, st in enumerate(steps):
        try:
            inputs = st.op.build(veteran, st.dtype, st.batch, st.nrhs, st.seed)
        except Exception as e:  # noqa: BLE001  (the message must carry the sequence)
            fail(k, "building the inputs", e)
        try:
            out_v = _run_one(veteran, st, inputs, hooks)
            _note(report, st, "veteran", st.op.check(inputs, out_v))
        except Exception as e:  # noqa: BLE001
            fail(k, "the veteran", e)
        if st.op.control:
            modes[st.op.name.split("=")[0]] = (st, inputs)
            continue

        def fresh_run():
            sol = make_solver()
            for cst, cin in modes.values():
                _run_one(sol, cst, cin, hooks)
            return _run_one(sol, st, inputs, hooks)
        try:
            out_f = fresh_run()
            _note(report, st, "fresh", st.op.check(inputs, out_f))
        except Exception as e:  # noqa: BLE001
            fail(k, "the fresh solver", e)
        if st.op.bitwise and compare:
            try:
                out_g = fresh_run()
                for key in st.op.bitwise:
                    assert _same_bits(out_f[key], out_g[key]), \
                        "two fresh solvers differ in %r: the operation is not reproducible, nothing can be " \
                        "said about history" % key
                    assert _same_bits(out_v[key], out_f[key]), \
                        "the veteran's %r is not bitwise the fresh solver's" % key
            except Exception as e:  # noqa: BLE001
                fail(k, "the veteran / fresh comparison", e)
    return veteran


def _note(report, step, who, ratios):
    if report is None or not ratios:
        return
    d = report.setdefault(step.op.family, {}).setdefault(who, {}).setdefault(np.dtype(step.dtype).name, {})
    for k, v in ratios.items():
        d[k] = max(d.get(k, 0.0), float(v))


# ---- structures ----------------------------------------------------------------------------------------

class Structure:
    """a solver factory with the host-side references of its matrices, computed once and shared: calling it
    gives a new Solver; `host` is one Solver that is only ever used for its layout on the host"""

    DATA_SEEDS = 3   # distinct matrices per kind and dtype (a step's seed picks one)

    def __init__(self, name, make):
        self.name, self._make, self._cache = name, make, {}

    def __call__(self):
        sol = self._make()
        sol._history = self
        return sol

    def cached(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    @property
    def host(self):
        return self.cached("host", self)

    @property
    def coords(self):
        return self.cached("coords", lambda: element_coords(self.host))

    @property
    def entries(self):
        return self.cached("entries", lambda: stored_entries(self.host))

    @property
    def splits(self):
        """admissible cuts of the partial operations (0 and numSpans() included)"""
        return self.cached("splits", lambda: [int(s) for s in splits(self.host)])

    def cut(self, seed, allow_end=True):
        """a cut picked by `seed`: an inner lump boundary where the structure has one"""
        sp = self.splits
        inner = sp[1:-1]
        if inner:
            return inner[seed % len(inner)]
        return sp[seed % len(sp)] if allow_end else sp[0]

    def kf(self, seed, dtype, rho=1.0):
        """known-factor data (known_factor.py); rho = 0.5: cond(A) < 100, the data of the adjoint tests"""
        def make():
            k = KF.known_factor_data(self.host, 100 + seed % self.DATA_SEEDS, dtype, rho=rho)
            if rho != 1.0:
                assert np.linalg.cond(k.A) < 100
            return k
        return self.cached(("kf", seed % self.DATA_SEEDS, np.dtype(dtype), rho), make)

    def spd(self, seed, dtype):
        """(data, A, inv(A)) of helpers.spd_data: the data of the selected-inversion and reach tests"""
        from helpers import spd_data

        def make():
            data = spd_data(self.host, 17 + seed % self.DATA_SEEDS, dtype=np.dtype(dtype).type)
            A, X, res = dense_reference(self.host, data)
            assert res < REF_RES, res
            return data, A, X
        return self.cached(("spd", seed % self.DATA_SEEDS, np.dtype(dtype)), make)

    def provided(self, what, seed, dtype, span=None):
        """a factor ("kf", "kf5", "spd"), partial factor ("partial", of kf5 up to `span`) or selected inverse
        ("selinv_kf5") computed on the device by a Solver of its own, which is neither a veteran nor a fresh
        one of any history; on the host"""
        def make():
            import torch
            from helpers import to_dev
            src = {"kf": lambda: self.kf(seed, dtype).data, "kf5": lambda: self.kf(seed, dtype, 0.5).data,
                   "partial": lambda: self.kf(seed, dtype, 0.5).data, "spd": lambda: self.spd(seed, dtype)[0],
                   "selinv_kf5": lambda: self.kf(seed, dtype, 0.5).data}[what]()
            sol = self._make()
            d = to_dev(src)
            if what == "partial":
                sol.factorUpTo(d, span)
            else:
                sol.factor(d)
            if what == "selinv_kf5":
                sol.selectedInverse(d)
            torch.cuda.synchronize()
            return d.cpu().numpy()
        return self.cached((what, seed % self.DATA_SEEDS, np.dtype(dtype), span), make)


def _S(solver):
    return solver._history


def _dev(a):
    from helpers import to_dev
    return to_dev(a)


def _arg(xs, batch):
    return list(xs) if batch > 1 else xs[0]


def _rhs(n, nrhs, dtype, seed):
    """n x nRHS right-hand sides, exactly representable in `dtype`"""
    return np.random.default_rng(seed).standard_normal((n, nrhs)).astype(dtype).astype(np.float64)


def _merge(*ratio_dicts):
    out = {}
    for r in ratio_dicts:
        for k, v in r.items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def _kf_check(errors, dtype, what):
    KF.check(errors, dtype, what)
    return KF.ratios(errors, dtype)


def _per_op(solver):
    return getattr(solver, "_history_per_op", False)


# ---- factor ------------------------------------------------------------------------------------------

def _build_factor(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    return {"dtype": dtype, "batch": batch, "kfs": [S.kf(seed + q, dtype) for q in range(batch)]}


def _run_factor(solver, i):
    devs = [_dev(k.data) for k in i["kfs"]]
    if _per_op(solver):  # (the per-op boundary is driven one matrix at a time)
        for d in devs:
            solver.factor(d)
    else:
        solver.factor(_arg(devs, i["batch"]))
    return {"data": devs}


def _check_factor(i, o):
    return _merge(*[_kf_check(k.factor_errors(d), i["dtype"], ("factor", q))
                    for q, (k, d) in enumerate(zip(i["kfs"], o["data"]))])


def _build_partial(solver, dtype, batch, nrhs, seed):
    i = _build_factor(solver, dtype, batch, nrhs, seed)
    S = _S(solver)
    i["span"] = S.cut(seed)
    i["bar"] = bar_of(S.host, i["span"])
    return i


def _run_partial(solver, i):
    devs = [_dev(k.data) for k in i["kfs"]]
    solver.factorUpTo(_arg(devs, i["batch"]), i["span"])
    mid = [d.clone() for d in devs]
    solver.factorFrom(_arg(devs, i["batch"]), i["span"])
    return {"partial": mid, "data": devs}


def _check_partial(i, o):
    rs = []
    for q, k in enumerate(i["kfs"]):
        k.check_partial(o["partial"][q], i["bar"], ("factorUpTo", i["span"], q))
        G = np.tril(k.sol.densify(o["partial"][q].astype(np.float64)))
        rs.append(KF.ratios(k.partial_errors_dense(G, i["bar"]), i["dtype"]))
        rs.append(_kf_check(k.factor_errors(o["data"][q]), i["dtype"], ("factorUpTo + factorFrom", i["span"], q)))
    return _merge(*rs)


def _run_factor_per_op(solver, i):
    devs = [_dev(k.data) for k in i["kfs"][:1]]
    with solver.forcePerOp():
        solver.factor(devs[0])
    if _per_op(solver):
        solver.forcePerOp(True)  # (the scope switched the mode of the walk off: back on)
    return {"data": devs}


# ---- solves ------------------------------------------------------------------------------------------

def _build_solve(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    n = S.host.order()
    return {"dtype": dtype, "batch": batch, "nrhs": nrhs, "n": n,
            "kfs": [S.kf(seed + q, dtype) for q in range(batch)],
            "L": [S.provided("kf", seed + q, dtype) for q in range(batch)],
            "b": [_rhs(n, nrhs, dtype, seed + q) for q in range(batch)]}


def _solve_args(i):
    mats = [_dev(L) for L in i["L"]]
    vecs = [_dev(b.T.ravel().astype(i["dtype"])) for b in i["b"]]
    ro = [("factor %d" % q, m, L) for q, (m, L) in enumerate(zip(mats, i["L"]))]
    return mats, vecs, ro


def _make_solve(method, op):
    def run(solver, i):
        mats, vecs, ro = _solve_args(i)
        getattr(solver, method)(_arg(mats, i["batch"]), _arg(vecs, i["batch"]), i["n"], i["nrhs"])
        return {"x": vecs, "_readonly": ro}

    def check(i, o):
        return _merge(*[_kf_check(k.solve_errors(b, KF.vec_to_cols(x, i["n"], i["nrhs"]), op), i["dtype"],
                                  (method, q)) for q, (k, b, x) in enumerate(zip(i["kfs"], i["b"], o["x"]))])
    return run, check


def _build_split(solver, dtype, batch, nrhs, seed):
    i = _build_solve(solver, dtype, batch, nrhs, seed)
    i["span"] = _S(solver).cut(seed)
    return i


def _make_split(first, second, op):
    def run(solver, i):
        mats, vecs, ro = _solve_args(i)
        for method in (first, second):
            getattr(solver, method)(_arg(mats, i["batch"]), i["span"], _arg(vecs, i["batch"]), i["n"], i["nrhs"])
        return {"x": vecs, "_readonly": ro}

    def check(i, o):
        return _merge(*[_kf_check(k.solve_errors(b, KF.vec_to_cols(x, i["n"], i["nrhs"]), op), i["dtype"],
                                  (first, second, i["span"], q))
                        for q, (k, b, x) in enumerate(zip(i["kfs"], i["b"], o["x"]))])
    return run, check


# ---- addMvFrom, pseudoFactorFrom ---------------------------------------------------------------------

def _build_addmv(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    n = S.host.order()
    sp = S.splits[:-1]
    span = sp[seed % len(sp)]
    return {"dtype": dtype, "nrhs": nrhs, "n": n, "kf": S.kf(seed, dtype), "span": span, "bar": bar_of(S.host, span),
            "vin": _rhs(n, nrhs, dtype, seed), "vout": _rhs(n, nrhs, dtype, seed + 1), "alpha": 0.75}


def _run_addmv(solver, i):
    dt = i["dtype"]
    dm, di, do = _dev(i["kf"].data), _dev(i["vin"].T.ravel().astype(dt)), _dev(i["vout"].T.ravel().astype(dt))
    solver.addMvFrom(dm, i["span"], di, i["n"], do, i["n"], i["nrhs"], i["alpha"])
    return {"out": do, "_readonly": [("matrix", dm, i["kf"].data), ("in", di, i["vin"].T.ravel().astype(dt))]}


def _check_addmv(i, o):
    """the statement of test_known_factor_gpu.test_add_mv_from"""
    bar, alpha, vin, vout = i["bar"], i["alpha"], i["vin"], i["vout"]
    got = KF.vec_to_cols(o["out"], i["n"], i["nrhs"])
    want = vout.copy()
    Ab = i["kf"].A[bar:, bar:]
    want[bar:] += alpha * (Ab @ vin[bar:])
    scale = alpha * np.linalg.norm(Ab) * np.linalg.norm(vin[bar:], axis=0) + np.linalg.norm(vout, axis=0)
    err = float(np.max(np.linalg.norm(got - want, axis=0) / scale))
    return _kf_check({"backward": err}, i["dtype"], ("addMvFrom", i["span"]))


def _build_pseudo(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    return {"dtype": dtype, "kf": S.kf(seed, dtype), "span0": (0, S.splits[len(S.splits) // 2] % S.host.numSpans())[seed % 2]}


def _run_pseudo(solver, i):
    d = _dev(i["kf"].data)
    solver.pseudoFactorFrom(d, i["span0"])
    return {"data": d}


def _check_pseudo(i, o):
    """the statement of test_known_factor_gpu.test_pseudo_factor_from"""
    kf, span0 = i["kf"], i["span0"]
    sol = kf.sol
    ss = sol.skel()["spanStart"]
    want = np.tril(kf.A)
    for j in range(span0, sol.numSpans()):
        a, b = int(ss[j]), int(ss[j + 1])
        Ld = np.linalg.cholesky(want[a:b, a:b])
        want[a:b, a:b] = Ld
        want[b:, a:b] = np.linalg.solve(Ld, want[b:, a:b].T).T
    got = np.tril(sol.densify(o["data"].astype(np.float64)))
    P = kf.pattern
    region = np.zeros_like(P)
    region[:, int(ss[span0]):] = True
    region &= P
    ref = want[region]
    err = float(np.linalg.norm(got[region] - ref) / np.linalg.norm(ref))
    keep = P & ~region
    assert np.array_equal(got[keep], np.tril(kf.A)[keep]), "pseudoFactorFrom changed a column before its span"
    return _kf_check({"off": err}, i["dtype"], ("pseudoFactorFrom", span0))


# ---- selected inversion, marginals --------------------------------------------------------------------

def _build_selinv(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    rng = np.random.default_rng(seed)
    ns = S.host.numSpans()
    return {"dtype": dtype, "batch": batch, "S": S, "X": [S.spd(seed + q, dtype)[2] for q in range(batch)],
            "L": [S.provided("spd", seed + q, dtype) for q in range(batch)],
            "params": sorted(int(p) for p in rng.choice(ns, size=min(ns, 5), replace=False))}


def _run_selinv(solver, i):
    zs = [_dev(L) for L in i["L"]]
    solver.selectedInverse(_arg(zs, i["batch"]))
    marg = [solver.marginals(z, i["params"]) for z in zs]
    return {"Z": zs, "marginals": [list(m) for m in marg]}


def _param_scalars(sol, prm):
    ss = sol.skel()["spanStart"]
    s = int(sol.paramToSpan()[prm])
    return np.arange(int(ss[s]), int(ss[s + 1]))


def _check_selinv(i, o):
    S, tol = i["S"], SELINV_TOL[np.dtype(i["dtype"])]
    worst = 0.0
    for q, (z, X) in enumerate(zip(o["Z"], i["X"])):
        err = corr_error(S.host, z.astype(np.float64), X, S.entries)
        assert err.value < tol, ("selectedInverse", q, err)
        worst = max(worst, err.value)
        d = np.diag(X)
        for p, blk in zip(i["params"], o["marginals"][q]):
            r = _param_scalars(S.host, p)
            e = float((np.abs(blk.astype(np.float64) - X[np.ix_(r, r)]) / np.sqrt(np.outer(d[r], d[r]))).max())
            assert e < tol, ("marginals", q, p, e)
            worst = max(worst, e)
    return {"selinv_corr": worst / tol}


# ---- logDet, factorStatus, dampDiagonal ---------------------------------------------------------------

def _build_status(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    ns = S.host.numSpans()
    b, e = ((0, ns), (min(1, ns), ns), (ns // 3, ns - ns // 4))[seed % 3]
    want = [np.linalg.slogdet(S.spd(seed + q, dtype)[1]) for q in range(batch)]
    assert all(s > 0 for s, _ in want)
    return {"dtype": dtype, "batch": batch, "S": S, "range": (b, e), "alpha": 0.125, "beta": 3.0,
            "data": [S.spd(seed + q, dtype)[0] for q in range(batch)], "logdet": [w for _, w in want],
            "L": [S.provided("spd", seed + q, dtype) for q in range(batch)]}


def _run_status(solver, i):
    (b, e), n = i["range"], i["batch"]
    Ls, ds, damped = [_dev(L) for L in i["L"]], [_dev(d) for d in i["data"]], [_dev(d) for d in i["data"]]
    ld = solver.logDet(_arg(Ls, n))
    st = solver.factorStatus(_arg(ds, n), b, e)
    solver.dampDiagonal(_arg(damped, n), i["alpha"], i["beta"], b, e)
    ro = [("factor %d" % q, t, h) for q, (t, h) in enumerate(zip(Ls, i["L"]))]
    ro += [("data %d" % q, t, h) for q, (t, h) in enumerate(zip(ds, i["data"]))]
    return {"logdet": ld.reshape(-1), "status": st.reshape(-1, 4), "damped": damped, "_readonly": ro}


def _check_status(i, o):
    S, (b, e), tol = i["S"], i["range"], LOGDET_TOL[np.dtype(i["dtype"])]
    worst = 0.0
    for q in range(i["batch"]):
        want = i["logdet"][q]
        err = abs(float(o["logdet"][q]) - want) / abs(want)
        assert err <= tol, ("logDet", q, float(o["logdet"][q]), want)
        worst = max(worst, err)
        assert np.array_equal(o["status"][q].astype(np.int64), scan_ref(S.host, i["data"][q], b, e)), ("factorStatus", q)
        assert KF.bitwise_equal(o["damped"][q], damp_ref(S.host, i["data"][q], i["alpha"], i["beta"], b, e)), \
            ("dampDiagonal", q)
    return {"logdet": worst / tol}


# ---- patternGrad, patternOuter -----------------------------------------------------------------------

def _build_pattern(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    n, ds, t = S.host.order(), S.host.dataSize(), np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    members = min(batch, 3)  # (member q of a larger batch holds the values of member q % 3)
    return {"dtype": dtype, "batch": batch, "k": nrhs, "S": S, "ld": n + 5, "n": n,
            "U": [rng.standard_normal((n, nrhs)).astype(t) for _ in range(members)],
            "V": [rng.standard_normal((n, nrhs)).astype(t) for _ in range(members)],
            "Z": [rng.standard_normal(ds).astype(t) for _ in range(members)],
            "s": [t(v) for v in (0.75, -1.0, 2.0)][:members],
            "Uo": [rng.uniform(-1, 1, (n, nrhs)).astype(t) for _ in range(members)],
            "Vo": [rng.uniform(-1, 1, (n, nrhs)).astype(t) for _ in range(members)]}


def _run_pattern(solver, i):
    import torch
    nb, k, n, ld, dt = i["batch"], i["k"], i["n"], i["ld"], i["dtype"]
    m = len(i["U"])
    tdt = torch.float64 if np.dtype(dt) == F64 else torch.float32

    def padded(a):
        t = torch.zeros((k, ld), dtype=tdt, device="cuda")
        t[:, :n] = _dev(np.ascontiguousarray(a.T))
        return t
    U, V = [padded(i["U"][q % m]) for q in range(nb)], [padded(i["V"][q % m]) for q in range(nb)]
    Z = [_dev(i["Z"][q % m]) for q in range(nb)]
    s = _dev(np.array([i["s"][q % m] for q in range(nb)], dtype=dt))
    ds = len(i["Z"][0])
    grad = [torch.full((ds,), float("nan"), dtype=tdt, device="cuda") for _ in range(nb)]
    solver.patternGrad(_arg(grad, nb), Z=_arg(Z, nb), zScale=s, U=_arg(U, nb), V=_arg(V, nb), nRHS=k, alpha=-1.5,
                       stride=ld)
    Uo, Vo = [_dev(np.ascontiguousarray(i["Uo"][q % m].T)) for q in range(nb)], \
        [_dev(np.ascontiguousarray(i["Vo"][q % m].T)) for q in range(nb)]
    outer = [torch.full((ds,), 7.0, dtype=tdt, device="cuda") for _ in range(nb)]
    solver.patternOuter(_arg(outer, nb), _arg(Uo, nb), _arg(Vo, nb), nRHS=k, alpha=-0.5)
    ro = [("Z %d" % q, Z[q], i["Z"][q % m]) for q in range(nb)]
    return {"grad": grad, "outer": outer, "_readonly": ro}


def _check_pattern(i, o):
    S, k, dt = i["S"], i["k"], np.dtype(i["dtype"])
    ci, cj = S.coords
    m = len(i["U"])
    wg, wo = [], []
    for q in range(m):
        wg.append(pattern_grad_ref(S.host, Z=i["Z"][q].astype(np.float64), s=float(i["s"][q]),
                                   U=i["U"][q].astype(np.float64), V=i["V"][q].astype(np.float64), alpha=-1.5,
                                   coords=S.coords))
        wo.append(np.where(ci >= cj, -0.5 * np.einsum("ek,ek->e", i["Uo"][q].astype(np.float64)[ci],
                                                      i["Vo"][q].astype(np.float64)[cj]), 0.0))
    worst_g = worst_o = 0.0
    for q in range(i["batch"]):
        got, want = o["grad"][q].astype(np.float64), wg[q % m]
        assert not np.isnan(got).any() and np.all(got[ci < cj] == 0), ("patternGrad", q)
        bound = PATTERN_GRAD_TOL[dt] * np.abs(want).max() * max(k, 1)
        err = np.abs(got - want).max()
        assert err <= bound, ("patternGrad", q, err, bound)
        worst_g = max(worst_g, err / bound)
        e = rel_error(o["outer"][q], wo[q % m])
        assert e < PATTERN_OUTER_TOL[dt], ("patternOuter", q, e)
        worst_o = max(worst_o, e / PATTERN_OUTER_TOL[dt])
    return {"pattern_grad": worst_g, "pattern_outer": worst_o}


# ---- adjoints ----------------------------------------------------------------------------------------

def _adjoint_ratio(name, got, want, dtype, what):
    tol = ADJOINT_TOL[np.dtype(dtype)]
    err = rel_error(got, want)
    assert np.isfinite(got).all() and err < tol, (name, what, err)
    return err / tol


def _build_factor_adjoint(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    t = np.dtype(dtype).type
    data = S.kf(seed, dtype, 0.5).data
    members = min(batch, 2)
    lbars = [lbar_random(S.host, seed + q, t) for q in range(members)]
    return {"dtype": dtype, "batch": batch, "S": S, "L": S.provided("kf5", seed, dtype), "lbar": lbars,
            "want": [dense_grad(S.host, data, lb, S.coords) for lb in lbars]}


def _run_factor_adjoint(solver, i):
    nb, m = i["batch"], len(i["lbar"])
    Ls = [_dev(i["L"]) for _ in range(nb)]
    gs = [_dev(i["lbar"][q % m]) for q in range(nb)]
    solver.factorAdjoint(_arg(Ls, nb), _arg(gs, nb))
    return {"grad": gs, "_readonly": [("factor %d" % q, L, i["L"]) for q, L in enumerate(Ls)]}


def _check_factor_adjoint(i, o):
    ci, cj = i["S"].coords
    m = len(i["lbar"])
    worst = 0.0
    for q, g in enumerate(o["grad"]):
        worst = max(worst, _adjoint_ratio("factorAdjoint", g, i["want"][q % m], i["dtype"], q))
        assert (g[ci < cj] == 0).all(), ("factorAdjoint", q)
    return {"factor_adjoint": worst}


def _build_partial_adjoint(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    t = np.dtype(dtype).type
    span = S.cut(seed)
    data = S.kf(seed, dtype, 0.5).data
    pbar = lbar_random(S.host, seed, t)
    P = S.provided("partial", seed, dtype, span)
    want, _ = partial_oracle(S.host, data, pbar, span, S.coords)
    bar = bar_of(S.host, span)
    schur = S.host.densify(P.astype(np.float64), fill_upper_half=True)[bar:, bar:].astype(t)
    return {"dtype": dtype, "batch": batch, "S": S, "span": span, "P": P, "pbar": pbar, "want": want, "schur": schur}


def _run_partial_adjoint(solver, i):
    nb = i["batch"]
    Ps = [_dev(i["P"]) for _ in range(nb)]
    gs = [_dev(i["pbar"]) for _ in range(nb)]
    solver.factorAdjointUpTo(_arg(Ps, nb), _arg(gs, nb), i["span"])
    out = {"grad": gs, "schur": [], "_readonly": [("P %d" % q, P, i["P"]) for q, P in enumerate(Ps)]}
    if i["schur"].size:
        sc = solver.schurComplement(_arg(Ps, nb), i["span"])
        out["schur"] = list(sc) if nb > 1 else [sc]
    return out


def _check_partial_adjoint(i, o):
    ci, cj = i["S"].coords
    worst = 0.0
    for q, g in enumerate(o["grad"]):
        worst = max(worst, _adjoint_ratio("factorAdjointUpTo", g, i["want"], i["dtype"], (i["span"], q)))
        assert (g[ci < cj] == 0).all(), ("factorAdjointUpTo", q)
    for q, sc in enumerate(o["schur"]):
        assert np.array_equal(sc, i["schur"]), ("schurComplement", i["span"], q)
    return {"partial_adjoint": worst}


def _build_selinv_adjoint(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    t = np.dtype(dtype).type
    data = S.kf(seed, dtype, 0.5).data
    grad = grad_random(S.host, seed, t)
    want = S.cached(("selinv_adjoint_want", seed % S.DATA_SEEDS, np.dtype(dtype), seed),
                    lambda: dense_lbar(S.host, dense_factor(S.host, data), grad, S.coords))
    return {"dtype": dtype, "batch": batch, "S": S, "L": S.provided("kf5", seed, dtype),
            "Z": S.provided("selinv_kf5", seed, dtype), "grad": grad, "want": want}


def _run_selinv_adjoint(solver, i):
    nb = min(i["batch"], 5)
    Ls, Zs = [_dev(i["L"]) for _ in range(nb)], [_dev(i["Z"]) for _ in range(nb)]
    gs = [_dev(i["grad"]) for _ in range(nb)]
    solver.selectedInverseAdjoint(_arg(Ls, nb), _arg(Zs, nb), _arg(gs, nb))
    ro = [("factor %d" % q, L, i["L"]) for q, L in enumerate(Ls)] + [("Z %d" % q, Z, i["Z"]) for q, Z in enumerate(Zs)]
    return {"grad": gs, "_readonly": ro}


def _check_selinv_adjoint(i, o):
    ci, cj = i["S"].coords
    worst = 0.0
    for q, g in enumerate(o["grad"]):
        worst = max(worst, _adjoint_ratio("selectedInverseAdjoint", g, i["want"], i["dtype"], q))
        assert (g[ci < cj] == 0).all(), ("selectedInverseAdjoint", q)
    return {"selinv_adjoint": worst}


# ---- reach solves ------------------------------------------------------------------------------------

def _build_reach(solver, dtype, batch, nrhs, seed):
    S = _S(solver)
    rng = np.random.default_rng(seed)
    ns = S.host.numSpans()
    prm = [int(p) for p in rng.choice(ns, size=min(ns, 6), replace=False)]
    data, A, X = S.spd(seed, dtype)
    return {"dtype": dtype, "S": S, "X": X, "A": A, "L": S.provided("spd", seed, dtype), "params": prm,
            "pairs": [(p, q) for p in prm for q in prm], "half": prm[:4] + prm[:1]}


def _run_reach(solver, i):
    L = _dev(i["L"])
    blocks = solver.inverseBlocks(L, i["pairs"])
    W = solver.halfInverseColumns(L, i["half"])
    return {"blocks": [b.reshape(-1) for b in blocks], "W": W, "_readonly": [("factor", L, i["L"])]}


def _check_reach(i, o):
    """the statements of test_inverse_blocks_gpu.py (_block_error, test_half_and_full_columns)"""
    S, X, tol = i["S"], i["X"], INVBLK_TOL[np.dtype(i["dtype"])]
    sol = S.host
    d = np.diag(X)
    worst = 0.0
    for (p, q), blk in zip(i["pairs"], o["blocks"]):
        r, c = _param_scalars(sol, p), _param_scalars(sol, q)
        got = blk.astype(np.float64).reshape(len(r), len(c))
        assert np.isfinite(got).all(), (p, q)
        worst = max(worst, float((np.abs(got - X[np.ix_(r, c)]) / np.sqrt(np.outer(d[r], d[c]))).max()))
    assert worst < tol, ("inverseBlocks", worst)
    Lc = S.cached(("chol", id(i["A"])), lambda: np.linalg.cholesky(i["A"]))
    idx = np.concatenate([_param_scalars(sol, p) for p in i["half"]])
    want = np.linalg.solve(Lc, np.eye(sol.order())[:, idx]).T
    W = o["W"].astype(np.float64)
    assert W.shape == want.shape
    half = float((np.abs(W - want) / np.sqrt(d[idx])[:, None]).max())
    assert half < tol, ("halfInverseColumns", half)
    return {"inverse_blocks": worst / tol, "half_columns": half / tol}


# ---- calls that raise, modes -------------------------------------------------------------------------

def _build_refused(solver, dtype, batch, nrhs, seed):
    """a cut that factorUpTo must refuse: inside a lump, or inside an elimination range"""
    S = _S(solver)
    bad = [s for s in range(1, S.host.numSpans()) if s not in S.splits]
    return {"dtype": dtype, "kf": S.kf(seed, dtype), "span": bad[seed % len(bad)] if bad else None}


def _run_refused(solver, i):
    d = _dev(i["kf"].data)
    raised = None
    try:
        if i["span"] is None:
            solver.factor(d[:-1])
        else:
            solver.factorUpTo(d, i["span"])
    except (RuntimeError, ValueError) as e:
        raised = e
    assert raised is not None, "factorUpTo(%s) was not refused" % i["span"]
    return {"_readonly": [("data", d, i["kf"].data)]}


def _nothing(*a):
    return {}


def _mode(name, apply):
    def run(solver, i):
        apply(solver)
        return {}
    return Op(name, "control", lambda *a: {}, run, _nothing, control=True)


def _set_per_op(on):
    def apply(solver):
        solver.forcePerOp(on)
        solver._history_per_op = on
    return apply


def _second_stream(solver):
    """a new stream that waits for the old one through an event (as test_inverse_blocks_gpu.py)"""
    import torch
    old = solver._torch_stream(torch.device("cuda", torch.cuda.current_device()))
    new = torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record(old)
    new.wait_event(ev)
    new.wait_stream(torch.cuda.current_stream())
    solver.setStream(new)


def _default_stream(solver):
    import torch
    old = solver._torch_stream(torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.default_stream().wait_stream(old)
    solver.setStream(None)


def _vocabulary():
    v = [Op("factor", "factor", _build_factor, _run_factor, _check_factor, uses_batch=True),
         Op("factorUpTo+factorFrom", "factor", _build_partial, _run_partial, _check_partial, uses_batch=True),
         Op("factor.perOp", "factor", _build_factor, _run_factor_per_op, _check_factor)]
    for method, op in (("solve", "A"), ("solveL", "L"), ("solveLt", "Lt")):
        run, check = _make_solve(method, op)
        v.append(Op(method, "solve", _build_solve, run, check, uses_batch=True, uses_nrhs=True))
    for first, second, op in (("solveLUpTo", "solveLFrom", "L"), ("solveLtFrom", "solveLtUpTo", "Lt")):
        run, check = _make_split(first, second, op)
        v.append(Op(first + "+" + second, "partial_solve", _build_split, run, check, uses_batch=True, uses_nrhs=True))
    v += [Op("addMvFrom", "addmv", _build_addmv, _run_addmv, _check_addmv, uses_nrhs=True),
          Op("pseudoFactorFrom", "addmv", _build_pseudo, _run_pseudo, _check_pseudo),
          Op("selectedInverse+marginals", "selinv", _build_selinv, _run_selinv, _check_selinv, bitwise=("Z", "marginals"),
             uses_batch=True),
          Op("logDet+factorStatus+dampDiagonal", "status", _build_status, _run_status, _check_status,
             bitwise=("logdet", "status", "damped"), uses_batch=True),
          Op("patternGrad+patternOuter", "pattern", _build_pattern, _run_pattern, _check_pattern,
             bitwise=("grad", "outer"), uses_batch=True, uses_nrhs=True),
          Op("factorAdjoint", "adjoint", _build_factor_adjoint, _run_factor_adjoint, _check_factor_adjoint,
             bitwise=("grad",), uses_batch=True),
          Op("factorAdjointUpTo+schurComplement", "adjoint", _build_partial_adjoint, _run_partial_adjoint,
             _check_partial_adjoint, bitwise=("grad", "schur"), uses_batch=True),
          Op("selectedInverseAdjoint", "adjoint", _build_selinv_adjoint, _run_selinv_adjoint, _check_selinv_adjoint,
             uses_batch=True),
          Op("inverseBlocks+halfInverseColumns", "reach", _build_reach, _run_reach, _check_reach,
             bitwise=("blocks", "W")),
          Op("refused", "error", _build_refused, _run_refused, _nothing),
          _mode("forcePerOp=1", _set_per_op(True)), _mode("forcePerOp=0", _set_per_op(False)),
          _mode("collectOpStats=1", lambda s: s.collectOpStats(True)),
          _mode("collectOpStats=0", lambda s: s.collectOpStats(False)),
          _mode("setStream=second", _second_stream), _mode("setStream=default", _default_stream)]
    return v


VOCABULARY = _vocabulary()
OPS = {op.name: op for op in VOCABULARY}


def steps_of(*specs):
    """steps from (name, dtype, batch, nrhs, seed) tuples"""
    return [Step(OPS[n], np.dtype(dt), b, r, s) for n, dt, b, r, s in specs]


# ---- the structures and the committed walks ------------------------------------------------------------

def _structures():
    import kf_structures as K
    from stress_cases import width_solver
    return collections.OrderedDict((s.name, s) for s in (
        Structure("tail", lambda: K.dense_solver(640)),                      # persistent tail, batch plan beside it
        Structure("sweep", lambda: width_solver(577, 70, hip_options={"sweep_min_width": 128})),  # sweeps, inverted blocks
        Structure("bipartite", lambda: K.bipartite(200, 9, 3, 6, 5)),        # elimination range, wide backward pass
        Structure("range", lambda: K.random_with_range(7)),                  # partial plans at lump boundaries
        Structure("widths", K.reach_widths)))                                # every path of the reach plan


STRUCTURES = _structures()

# Seeds of the random walks per structure, chosen on the host (tests/test_history_cpu.py asserts what they
# cover: every ordered pair of required families over all of them; both dtype switches, a batch decrease
# and an nRHS decrease on each structure)
WALK_LENGTH = 20
WALK_SEEDS = {"tail": [5331, 2530, 20], "sweep": [503, 1], "bipartite": [409, 2], "range": [4412, 3], "widths": [6819, 6]}


def committed_walks(vocabulary=None):
    """{structure name: [(seed, steps)]}"""
    vocabulary = VOCABULARY if vocabulary is None else vocabulary
    return {name: [(s, random_history(s, WALK_LENGTH, vocabulary)) for s in seeds] for name, seeds in WALK_SEEDS.items()}
