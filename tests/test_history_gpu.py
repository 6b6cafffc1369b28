"""GPU: a Solver's results do not depend on what it was used for before (tests/history.py).

Fixed scenarios reach each piece of state that survives a call (csrc/hip_context.h) and assert by the run
counters that the path was the one meant; random walks (seeds committed in history.WALK_SEEDS, their
coverage asserted on the host by tests/test_history_cpu.py) mix every family of operations, both
precisions, batch sizes, right-hand-side counts, the per-op mode, op statistics and a second stream on one
long-lived Solver.  Every operation is checked against its existing high-precision reference at its
existing tolerance on the veteran and on a fresh Solver; the bitwise reproducible operations must give the
veteran and the fresh Solver the same bits.

HISTORY_REPORT=<path>: the worst error / tolerance per family, dtype and metric of the veteran and of the
fresh solvers is written there as JSON when the process ends (as KNOWN_FACTOR_REPORT of known_factor.py).

Nothing here makes a kernel spin, time out or fault: the error scenarios use argument checks, a matrix that
is not positive definite (the factor then holds NaN and factorStatus says where) and factorRegularized."""
import atexit
import json
import os

import numpy as np
import pytest

import baspacho_amd as B
import history as H
import kf_structures as K
from factor_status_ref import damp as damp_ref
from helpers import spd_data, to_dev
from history import F32, F64, steps_of
from known_factor import bitwise_equal, known_factor_data, vec_to_cols

pytestmark = pytest.mark.gpu

S = H.STRUCTURES
REPORT = {}
_REPORT_PATH = os.environ.get("HISTORY_REPORT")


@atexit.register
def _write_report():
    if _REPORT_PATH and REPORT:
        with open(_REPORT_PATH, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


class Counted:
    """a solver factory that hands out `solver` first (the veteran of run_history) and new ones afterwards"""

    def __init__(self, structure, solver=None):
        self.structure, self.first = structure, solver

    def __call__(self):
        sol, self.first = (self.first, None) if self.first is not None else (self.structure(), None)
        return sol


def _run(structure, specs, tag, veteran=None):
    return H.run_history(Counted(structure, veteran), steps_of(*specs), tag=tag, report=REPORT)


def _delta(sol, fn):
    before = sol.runCounters()
    fn()
    after = sol.runCounters()
    return {k: after[k] - before[k] for k in after}


def _alternating(name_args, dtypes=(F64, F32, F64, F32), seed=11):
    """every (name, batch, nrhs) of `name_args` in each of `dtypes` in turn"""
    return [(n, dt, b, r, seed + k) for k, dt in enumerate(dtypes) for n, b, r in name_args]


# ---- precision alternation -----------------------------------------------------------------------------

PRECISION_OPS = [("factor", 1, 1), ("solve", 1, 17), ("solve", 1, 1), ("selectedInverse+marginals", 1, 1),
                 ("factorAdjoint", 1, 1), ("inverseBlocks+halfInverseColumns", 1, 1)]


@pytest.mark.parametrize("name", ["tail", "sweep", "bipartite"])
def test_precision_alternation(name):
    """fp64, fp32, fp64, fp32 through factor, solve at nRHS 17 then 1, selected inverse, factor adjoint and
    inverseBlocks on one solver: the scratch that both precisions share through casts (dinvScratch, tailCtl,
    tailDinv, solveInvScratch, solveWideBuf, sweepXchg), sweepAttr per value size, the selected-inversion and
    reach scratch"""
    sol = S[name]()
    d = _delta(sol, lambda: _run(S[name], _alternating(PRECISION_OPS), "precision/" + name, veteran=sol))
    print("precision", name, d)
    if name == "tail":
        assert sol.planStats()["num_tail_panels"] > 0 and d["tail_launches"] == 4, d  # one per factor, both dtypes
    if name == "sweep":
        assert d["sweep_launches"] >= 4, d                            # the solves of both dtypes took the sweeps
    if name == "bipartite":
        assert d["solve_wide_launches"] >= 4, d                        # nRHS 17 in both dtypes: the wide backward pass
    assert d["selinv_launches"] > 0 and d["sweep_timeouts"] == 0 and d["sweep_error_pending"] == 0, d


# ---- shrinking calls -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["tail", "sweep", "bipartite"])
def test_shrinking_batches_and_rhs_counts(name, dtype):
    """batch 17, 1, 5 and nRHS 17, 1, 16, 3: a grown buffer keeps stale contents behind the part that the
    smaller call arms"""
    sol = S[name]()
    specs = [("factor", dtype, b, 1, 20 + b) for b in (17, 1, 5)]
    specs += [("solve", dtype, b, 3, 30 + b) for b in (17, 1, 5)]
    specs += [(m, dtype, 1, r, 40 + r) for r in (17, 1, 16, 3) for m in ("solve", "solveL", "solveLt")]
    specs += [("solveLUpTo+solveLFrom", dtype, b, r, 50 + r) for b, r in ((5, 17), (1, 1), (2, 16), (1, 3))]
    specs += [("selectedInverse+marginals", dtype, b, 1, 60 + b) for b in (5, 1, 2)]
    d = _delta(sol, lambda: _run(S[name], specs, "shrinking/%s/%s" % (name, dtype.name), veteran=sol))
    print("shrinking", name, dtype.name, d)
    if name == "tail":
        assert d["tail_launches"] == 1, d          # the single factor between the two batches took the tail
    if name == "bipartite":
        assert d["solve_wide_launches"] >= 1, d
    if name == "sweep":
        assert d["sweep_launches"] >= 1, d
    assert d["selinv_chunks"] >= 3, d


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_matrix_core_sweep_around_the_scalar_one(monkeypatch, dtype):
    """the matrix-core sweep (groups of 16 right-hand sides), the scalar one (up to 16), the matrix-core one
    again: both size sweepXchg and the inverted blocks for themselves"""
    monkeypatch.setenv("BSP_SWEEP_MFMA_MIN", "3")
    monkeypatch.setenv("BSP_SWEEP_MFMA_MIN_WIDTH", "0")
    sol = S["sweep"]()
    seen = []
    for nrhs, counter in ((17, "sweep_mfma_launches"), (1, "sweep_launches"), (16, "sweep_mfma_launches"),
                          (2, "sweep_launches"), (17, "sweep_mfma_launches")):
        for method in ("solve", "solveLt"):
            d = _delta(sol, lambda: _run(S["sweep"], [(method, dtype, 1, nrhs, 70 + nrhs)], "mfma-sweep", veteran=sol))
            seen.append((nrhs, method, d["sweep_mfma_launches"], d["sweep_launches"]))
            # (a matrix-core sweep counts as a sweep as well)
            assert d["sweep_launches"] >= 1 and (d["sweep_mfma_launches"] >= 1) == (counter == "sweep_mfma_launches"), \
                (nrhs, method, counter, d)
    print("mfma / scalar sweeps", dtype.name, seen)


# ---- sub-batches ---------------------------------------------------------------------------------------

@pytest.mark.product_defaults  # (a batch is split only when its plan hands no lookahead units to the side streams)
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_sub_batches_then_the_tail_then_sub_batches(monkeypatch, dtype):
    """a batch factored as concurrent sub-batches (the batch plan, the shared batch streams), a single
    matrix (the persistent tail of the single plan), the batch again"""
    monkeypatch.setenv("BSP_SUB_BATCH_MIN", "2")
    sol = S["tail"]()
    deltas = []
    for k, batch in enumerate((4, 1, 4)):
        deltas.append(_delta(sol, lambda: _run(S["tail"], [("factor", dtype, batch, 1, 80 + k),
                                                           ("solve", dtype, batch, 3, 90 + k)],
                                               "sub-batches", veteran=sol)))
    print("sub-batches", dtype.name, [(d["sub_batches_enqueued"], d["tail_launches"]) for d in deltas])
    assert deltas[0]["sub_batches_enqueued"] >= 2 and deltas[2]["sub_batches_enqueued"] >= 2, deltas
    assert deltas[1]["tail_launches"] == 1 and deltas[1]["sub_batches_enqueued"] == 0, deltas
    assert deltas[0]["tail_launches"] == 0 and deltas[2]["tail_launches"] == 0, deltas


# ---- several spans -------------------------------------------------------------------------------------

def _seeds_for_cuts(structure, want):
    """step seeds whose Structure.cut() gives the first `want` different inner cuts"""
    out, seen = [], set()
    for seed in range(200):
        c = structure.cut(seed)
        if c not in seen:
            seen.add(c)
            out.append(seed)
        if len(out) == want:
            return out, sorted(seen)
    raise AssertionError("the structure has fewer than %d inner cuts" % want)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_partial_plans_at_three_spans(dtype):
    """factorUpTo / factorFrom, solveLUpTo / solveLFrom and addMvFrom at three lump boundaries between full
    factors: the plans keyed by (tag, begin, end), the solve gather lists and the addMv tile lists per range"""
    st = S["range"]
    seeds, cuts = _seeds_for_cuts(st, 3)
    assert len(cuts) == 3 and all(0 < c < st.host.numSpans() for c in cuts)
    specs = []
    for s in seeds + seeds[:1]:  # (the first cut again at the end: its plans are now old)
        specs += [("factor", dtype, 1, 1, s), ("factorUpTo+factorFrom", dtype, 1, 1, s),
                  ("solveLUpTo+solveLFrom", dtype, 1, 3, s), ("solveLtFrom+solveLtUpTo", dtype, 2, 1, s),
                  ("addMvFrom", dtype, 1, 3, s), ("factorUpTo+factorFrom", dtype, 2, 1, s)]
    # addMvFrom takes its span from splits[:-1] by the seed: three different ones as well
    spans = {st.splits[:-1][s % len(st.splits[:-1])] for s in seeds}
    assert len(spans) == 3, spans
    _run(st, specs, "spans/" + dtype.name)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_partial_adjoints_at_two_spans(dtype):
    """factorAdjointUpTo and schurComplement at two lump boundaries between full factors and full adjoints:
    the selected-inversion plans per cut (selinvUpTo) beside the full one"""
    st = S["range"]
    seeds, cuts = _seeds_for_cuts(st, 2)
    sol = st()
    specs = []
    for s in seeds + seeds:
        specs += [("factor", dtype, 1, 1, s), ("factorAdjointUpTo+schurComplement", dtype, 1, 1, s),
                  ("factorAdjoint", dtype, 1, 1, s), ("factorAdjointUpTo+schurComplement", dtype, 2, 1, s)]
    _run(st, specs, "adjoint-spans/" + dtype.name, veteran=sol)
    # no counter tells the cuts apart: the plans that the two cuts run (built by the function the device path
    # uses) differ from each other and are shorter than the full one
    def records(plan):
        return len(plan["small"]["lump"]) + len(plan["node"]["lump"])
    sizes = [records(sol._testSelInvPlan(c)) for c in cuts]
    assert 0 < sizes[0] < sizes[1] < records(sol._testSelInvPlan()), sizes


# ---- first-use order -----------------------------------------------------------------------------------

FIRST = ["selectedInverseAdjoint", "inverseBlocks+halfInverseColumns", "patternGrad+patternOuter", "solveLt"]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("first", FIRST)
def test_first_use_order(first, dtype):
    """the first call on a new Solver is an extension operation (or a batched solveLt on a second stream) on a
    factor that another Solver computed: the extension state, the code objects of the solve and extension
    units and the skeleton mirror are built by it, not by a factor; then the usual factor and solve"""
    st = S["sweep"]
    specs = []
    if first == "solveLt":
        specs.append(("setStream=second", dtype, 1, 1, 1))
    specs += [(first, dtype, 3 if first == "solveLt" else 1, 3, 5), ("factor", dtype, 1, 1, 6), ("solve", dtype, 1, 3, 7),
              ("selectedInverse+marginals", dtype, 1, 1, 8)]
    sol = st()
    _run(st, specs, "first-use/%s/%s" % (first, dtype.name), veteran=sol)
    if first == "solveLt":
        sol.setStream(None)


# ---- the pointer ring ----------------------------------------------------------------------------------

def _tiny():
    return K.dense_solver(24, span=3)


def _batched_solve_inputs(sol, dtype, batch, nrhs, seed, L):
    n = sol.order()
    bs = [np.random.default_rng(seed + q).standard_normal((n, nrhs)).astype(dtype).astype(np.float64)
          for q in range(batch)]
    return bs, [to_dev(L) for _ in range(batch)], [to_dev(b.T.ravel().astype(dtype)) for b in bs]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_ring_wrap(dtype):
    """40 batched solves queued on one Solver with no host synchronisation in between: the ring of 32 pointer
    slots wraps, and a slot is rewritten only after its call's kernels"""
    import torch
    sol = _tiny()
    kf = known_factor_data(sol, 3, dtype)
    L = to_dev(kf.data)
    _tiny().factor(L)  # (another Solver's factor)
    L = L.cpu().numpy()
    n, nrhs = sol.order(), 3
    calls = [_batched_solve_inputs(sol, dtype, 2 + k % 3, nrhs, 1000 + 10 * k, L) for k in range(40)]
    torch.cuda.synchronize()
    assert sol._testPtrRingSlotBytes() == 0
    for bs, mats, vecs in calls:
        sol.solve(mats, vecs, n, nrhs)
    assert sol._testPtrRingSlotBytes() == 512  # 64 pointers: never grown
    torch.cuda.synchronize()
    for k, (bs, mats, vecs) in enumerate(calls):
        for q, (b, v) in enumerate(zip(bs, vecs)):
            kf.check_solve(b, vec_to_cols(v.cpu().numpy(), n, nrhs), "A", ("ring wrap", k, q))
            assert bitwise_equal(mats[q].cpu().numpy(), L)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_ring_growth(dtype):
    """batches of 3 and 64 fit the first slots; a batch of 65 right behind a queued batch of 3 makes the ring
    wait for the device, free every slot and allocate larger ones: both calls and the next batch of 3 are right.
    The slot size (bsp_test_ptr_ring_slot_bytes) is the only sign that the growth path ran"""
    import torch
    sol = _tiny()
    n, nrhs = sol.order(), 3
    kfs = [known_factor_data(sol, 10 + q, dtype) for q in range(5)]
    provider = _tiny()
    Ls = []
    for k in kfs:
        d = to_dev(k.data)
        provider.factor(d)
        Ls.append(d.cpu().numpy())

    def check_factor(devs, what):
        for q, d in enumerate(devs):
            kfs[q % 5].check_factor(d.cpu().numpy(), (what, q))

    def check_solve(bs, vecs, what):
        for q, (b, v) in enumerate(zip(bs, vecs)):
            kfs[q].check_solve(b, vec_to_cols(v.cpu().numpy(), n, nrhs), "A", (what, q))

    def inputs(batch):
        return [to_dev(kfs[q % 5].data) for q in range(batch)]

    def solve_inputs(seed):
        calls = [_batched_solve_inputs(sol, dtype, 1, nrhs, seed + q, Ls[q]) for q in range(3)]
        return [c[0][0] for c in calls], [c[1][0] for c in calls], [c[2][0] for c in calls]

    # every buffer is on the device before the calls under test are queued: an upload in between would wait
    # for the stream
    small, full, grown, again = inputs(3), inputs(64), inputs(65), inputs(3)
    queued, after = solve_inputs(100), solve_inputs(200)
    torch.cuda.synchronize()
    sol.factor(small)
    sol.factor(full)
    assert sol._testPtrRingSlotBytes() == 512
    sol.solve(queued[1], queued[2], n, nrhs)   # still queued when ...
    sol.factor(grown)                          # ... the ring grows
    assert sol._testPtrRingSlotBytes() == 768, "the growth path of the ring did not run"
    sol.solve(after[1], after[2], n, nrhs)
    sol.factor(again)
    assert sol._testPtrRingSlotBytes() == 768
    torch.cuda.synchronize()
    check_factor(small, "batch 3")
    check_factor(full, "batch 64")
    check_solve(queued[0], queued[2], "batch 3 before the growth")
    check_factor(grown, "batch 65")
    check_solve(after[0], after[2], "batch 3 after the growth")
    check_factor(again, "batch 3 after the growth")


# ---- after an error ------------------------------------------------------------------------------------

RECOVERY = [("factor", 1, 1), ("solve", 1, 3), ("selectedInverse+marginals", 1, 1), ("factor", 2, 1), ("solve", 2, 17)]


def _indefinite(sol, seed, dtype):
    """helpers.spd_data shifted so that its smallest eigenvalue is -1e-3 max diag (test_factor_status_gpu.py)"""
    Bd = spd_data(sol, seed, dtype=dtype.type)
    diag = sol.diagOffsets()
    lam = np.linalg.eigvalsh(sol.densify(Bd.astype(np.float64), fill_upper_half=True))[0]
    delta = 1e-3 * float(Bd[diag].max())
    A = Bd.copy()
    A[diag] = (Bd[diag].astype(np.float64) - (lam + delta)).astype(dtype)
    return A, delta


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["tail", "bipartite", "range"])
def test_after_an_error(name, dtype):
    """a call refused by an argument check, a factor that breaks down (NaN in the data, reported by
    factorStatus) and a factorRegularized that retries: after each, factor, solve and selected inverse of valid
    inputs pass their checks on the same Solver"""
    import torch
    st = S[name]
    sol = st()
    host = st.host
    n, ns = host.order(), host.numSpans()

    def recover(tag, seed):
        _run(st, [(op, dtype, b, r, seed + k) for k, (op, b, r) in enumerate(RECOVERY)],
             "after-error/%s/%s/%s" % (name, dtype.name, tag), veteran=sol)

    recover("before", 1)
    # 1. argument checks: a length, a cut that is refused, a span range
    _run(st, [("refused", dtype, 1, 1, 3)], "refused", veteran=sol)
    d = to_dev(st.kf(0, dtype).data)
    with pytest.raises(ValueError):
        sol.solve(d[:-1], d[:n], n, 1)
    with pytest.raises(ValueError):
        sol.factorStatus(d, 2, ns + 1)
    with pytest.raises((RuntimeError, ValueError)):
        sol.patternGrad(d)  # neither Z nor U / V
    recover("refused", 10)
    # 2. a symmetric matrix that is not positive definite
    A, delta = _indefinite(host, 61, dtype)
    dev = to_dev(A)
    sol.factor(dev)
    status = sol.readFactorStatus(sol.factorStatus(dev))
    got = dev.cpu().numpy()
    print("breakdown", name, dtype.name, status)
    assert not status["ok"] and status["count"] >= 1 and 0 <= status["first"] < n
    assert np.isnan(got[host.diagOffsets()[status["first"]]]) or got[host.diagOffsets()[status["first"]]] <= 0
    recover("breakdown", 20)
    # 3. a regularised factor that retries three times
    devA = to_dev(A)
    out, info = sol.factorRegularized(devA, alpha=0.0, beta0=delta / 30, growth=10.0)
    torch.cuda.synchronize()
    assert info["retries"] == 3 and info["status"]["ok"], info
    assert bitwise_equal(devA.cpu().numpy(), A), "A was written"
    damped = damp_ref(host, A, 0.0, dtype.type(info["beta"]))
    rhs = np.random.default_rng(7).standard_normal(n).astype(dtype)
    v = to_dev(rhs)
    sol.solve(out, v, n, 1)
    X = np.linalg.solve(host.densify(damped.astype(np.float64), fill_upper_half=True), rhs.astype(np.float64))
    err = np.linalg.norm(v.cpu().numpy().astype(np.float64) - X) / np.linalg.norm(X)
    assert err < (1e-10 if dtype == F64 else 1e-3), err  # (the bound of test_factor_status_gpu.py)
    with pytest.raises(B.FactorizationError):
        sol.factorRegularized(devA, alpha=0.0, beta0=delta / 30, growth=10.0, maxRetries=1)
    recover("regularised", 30)
    c = sol.runCounters()
    assert c["sweep_timeouts"] == 0 and c["sweep_error_pending"] == 0, c


# ---- random walks --------------------------------------------------------------------------------------

WALKS = [(name, seed) for name, seeds in H.WALK_SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("name,seed", WALKS, ids=["%s-%d" % w for w in WALKS])
def test_random_walk(name, seed):
    steps = H.random_history(seed, H.WALK_LENGTH, H.VOCABULARY)
    print("\n".join(H.describe(steps)))
    sol = H.run_history(S[name], steps, tag="walk/%s/%d" % (name, seed), report=REPORT)
    sol.setStream(None)
    c = sol.runCounters()
    assert c["sweep_timeouts"] == 0 and c["sweep_error_pending"] == 0, c
