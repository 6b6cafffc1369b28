"""GPU: factor and solve kernels on known-factor data (tests/known_factor.py) at tolerances scaled to
the working precision, along the kernel edges: lump widths around every tile / panel / block size,
the persistent tail, folded potrf, split-K, lookahead, batches and sub-batches, every sparse-
elimination factor and update kernel, the per-op path, right-hand-side counts around the groups of 8
and 16, sweeps, the wide / inverse / block solve switches, batched and partial solves, addMvFrom and
pseudoFactorFrom.  The fault-injection test shows that the checks notice a dropped update at small
size.  The run counters assert that the path under test was the one taken."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from helpers import solver_random, to_dev
from known_factor import check, known_factor_data, stored_pattern, tolerance, vec_to_cols
from kf_structures import bipartite as _bipartite
from kf_structures import blocks_over_separator as _blocks_over_separator
from kf_structures import counter_delta as _counter_delta
from kf_structures import dense_solver as _dense_solver
from kf_structures import random_with_range as _random_with_range
from stress_cases import width_solver

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def _factor(sol, dtype, seed, what=""):
    kf = known_factor_data(sol, seed, dtype)
    dev = to_dev(kf.data)
    sol.factor(dev)
    kf.check_factor(dev.cpu().numpy(), what)
    return kf, dev


def _rhs(n, nrhs, dtype, seed):
    """n x nRHS right-hand sides, exactly representable in `dtype`"""
    return np.random.default_rng(seed).standard_normal((n, nrhs)).astype(dtype).astype(np.float64)


def _solve(kf, dev, nrhs, op="A", seed=1, what=""):
    sol, n, dtype = kf.sol, kf.sol.order(), kf.dtype
    b = _rhs(n, nrhs, dtype, seed)
    v = to_dev(b.T.ravel().astype(dtype))
    getattr(sol, {"A": "solve", "L": "solveL", "Lt": "solveLt"}[op])(dev, v, n, nrhs)
    kf.check_solve(b, vec_to_cols(v.cpu().numpy(), n, nrhs), op, (what, op, nrhs))


# ---- lump widths ------------------------------------------------------------------------------

WIDTH_GROUPS = [(1, 2, 3, 4, 5, 6, 7, 8, 9), (15, 16, 17), (31, 32, 33), (63, 64, 65), (127, 128, 129),
                (191, 192, 193), (255, 256, 257), (511, 512, 513), (1023, 1024, 1025)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("widths", WIDTH_GROUPS, ids=lambda g: "W%d-%d" % (g[0], g[-1]))
def test_lump_widths(widths, dtype):
    """run_width_case's structure: a dense lump of width W, alone and with a 70-column lump below"""
    for W in widths:
        for tail in (0, 70):
            sol = width_solver(W, tail)
            kf, dev = _factor(sol, dtype, 5 + W, ("W", W, tail))
            _solve(kf, dev, 1, seed=W, what=("W", W, tail))


# ---- schedule variants of the dense phase -----------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tail", ["on", "off"])
def test_persistent_tail(monkeypatch, tail, dtype):
    """wide roots (1599, 2049: tail of 4 outer blocks) and narrow ones (640, 990: all but the first
    outer block), with the tail launch and without it"""
    for W, blocks in ((1599, 4), (2049, 4), (640, -1), (990, -1)):
        opts = {"tail_blocks": 0} if tail == "off" else ({"tail_blocks": blocks} if blocks > 0 else None)
        sol = _dense_solver(W, span=8 if W % 2 == 0 else 7, hip_options=opts)
        kf = known_factor_data(sol, 3 + W, dtype)
        dev = to_dev(kf.data)
        took = _counter_delta(sol, "tail_launches", lambda: sol.factor(dev))
        assert (took == 1) == (tail == "on"), (W, took)
        kf.check_factor(dev.cpu().numpy(), ("tail", tail, W))
        _solve(kf, dev, 2, seed=W, what=("tail", tail, W))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fold", ["1", "0"])
def test_folded_potrf(monkeypatch, fold, dtype):
    monkeypatch.setenv("BSP_POTRF_IN_TRSM", fold)
    sol = _blocks_over_separator([130, 97, 200, 70], 150)
    for bs in (1, 3):
        kfs = [known_factor_data(sol, 90 + q, dtype) for q in range(bs)]
        devs = [to_dev(k.data) for k in kfs]
        folded = _counter_delta(sol, "potrf_folded_levels", lambda: sol.factor(devs if bs > 1 else devs[0]))
        assert (folded > 0) == (fold == "1"), folded
        for k, d in zip(kfs, devs):
            k.check_factor(d.cpu().numpy(), ("fold", fold, bs))
        _solve(kfs[0], devs[0], 1, what=("fold", fold))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", ["1", "0"])
def test_split_k(monkeypatch, split, dtype):
    monkeypatch.setenv("BSP_SPLIT_K", split)
    sol = _blocks_over_separator([130, 130, 200, 200], 150)
    for bs in (1, 3):
        kfs = [known_factor_data(sol, 70 + q, dtype) for q in range(bs)]
        devs = [to_dev(k.data) for k in kfs]
        used = _counter_delta(sol, "split_lists_used", lambda: sol.factor(devs if bs > 1 else devs[0]))
        assert (used > 0) == (split == "1"), used
        for k, d in zip(kfs, devs):
            k.check_factor(d.cpu().numpy(), ("split-K", split, bs))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ahead", ["0", "0.6", "100"])
def test_lookahead(monkeypatch, ahead, dtype):
    """a dense lump of seven outer blocks with a ragged last one (lookahead units on the side stream)"""
    monkeypatch.setenv("BSP_BULK_AHEAD", ahead)
    n = 1700
    sol = B.create_solver(B.Settings(hipOptions={"tail_blocks": 0}), np.ones(n, dtype=np.int64),
                          T.columns_to_structure([set(range(i, n)) for i in range(n)]))
    kf = known_factor_data(sol, 23, dtype)
    dev = to_dev(kf.data)
    forks = _counter_delta(sol, "lookahead_forks", lambda: sol.factor(dev))
    assert forks > 0, forks
    kf.check_factor(dev.cpu().numpy(), ("ahead", ahead))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [1, 2, 5, 17])
def test_batched_factor(bs, dtype):
    """each matrix of the batch with its own L0; a wide lump, a narrow tree and an elimination range"""
    for sol in (width_solver(300, 70), _bipartite(200, 9, 3, 6, seed=bs)):
        kfs = [known_factor_data(sol, 1000 * bs + q, dtype) for q in range(bs)]
        devs = [to_dev(k.data) for k in kfs]
        sol.factor(devs)
        for q, (k, d) in enumerate(zip(kfs, devs)):
            k.check_factor(d.cpu().numpy(), ("batch", bs, q))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [4, 17])
def test_forced_sub_batches(monkeypatch, bs, dtype):
    monkeypatch.setenv("BSP_SUB_BATCH_MIN", "2")
    sol = _blocks_over_separator([130, 97, 200, 70], 150)
    kfs = [known_factor_data(sol, 500 + q, dtype) for q in range(bs)]
    devs = [to_dev(k.data) for k in kfs]
    parts = _counter_delta(sol, "sub_batches_enqueued", lambda: sol.factor(devs))
    assert parts >= 2, parts
    for q, (k, d) in enumerate(zip(kfs, devs)):
        k.check_factor(d.cpu().numpy(), ("sub-batch", bs, q))


# ---- sparse elimination -----------------------------------------------------------------------

# (pt_size, cam_size): elimination lumps <= 4 wide (elimFactorTinyStaged), <= 8 (elimFactorSmall<8>),
# <= 16 (elimFactorSmall<16>), > 16 (dense levels inside the range); target blocks of <= 9 elements with
# a narrow source (elimGatherTiny<9>), of <= 16 (elimGatherTiny<16>), up to 16 x 16 (elimGatherMfma),
# and camera blocks of more than 256 elements (no gather: the chain update elimUpdate)
# (number of points, pt_size, cam_size)
ELIM_CASES = {"tiny9": (400, 3, 3), "tiny16": (400, 4, 4), "mfma_w6": (300, 6, 9), "mfma_w12": (150, 12, 7),
              "mfma_w20": (100, 20, 6), "chain_w3": (400, 3, 17), "chain_w7": (250, 7, 18)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(ELIM_CASES))
def test_sparse_elimination(case, dtype):
    pts, pt, cam = ELIM_CASES[case]
    sol = _bipartite(pts, 13, pt, cam, seed=pt * 31 + cam)
    assert len(sol.sparseEliminationRanges()) >= 2
    kf, dev = _factor(sol, dtype, 17 + pt, ("elim", case))
    _solve(kf, dev, 1, seed=pt, what=("elim", case))
    _solve(kf, dev, 5, seed=pt, what=("elim", case))


@pytest.mark.parametrize("dtype", DTYPES)
def test_automatic_elimination_ranges(dtype):
    """ranges found by the solver on a random structure (mixed lump widths in one range)"""
    cols = T.make_independent_elim_set(T.random_cols(400, 0.02, 5), 0, 250)
    sizes = np.random.default_rng(5).integers(1, 6, size=400).astype(np.int64)
    sol = B.create_solver(B.Settings(), sizes, T.columns_to_structure(cols), [])
    assert len(sol.sparseEliminationRanges()) >= 2
    kf, dev = _factor(sol, dtype, 8, "auto ranges")
    _solve(kf, dev, 3, what="auto ranges")


def test_fault_injection_is_flagged():
    """_testSetFault(1) drops the sparse-elimination update: the known-factor check fails at small size,
    by far, and passes once the fault is off"""
    sol = _bipartite(120, 7, 3, 6, seed=4)
    kf = known_factor_data(sol, 2, np.float64)
    dev = to_dev(kf.data)
    sol._testSetFault(1)
    try:
        sol.factor(dev)
    finally:
        sol._testSetFault(0)
    errs = kf.factor_errors(dev.cpu().numpy())
    assert errs["off"] > 1e6 * tolerance("off", np.float64), errs
    with pytest.raises(AssertionError):
        kf.check_factor(dev.cpu().numpy())
    dev = to_dev(kf.data)
    sol.factor(dev)
    kf.check_factor(dev.cpu().numpy())


# ---- per-op path ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_per_op_path(dtype):
    """factor and solves through the op-by-op loops: merged lumps of several spans (the per-op solve
    virtuals), an elimination range, a wide lump"""
    merged, _, _ = solver_random(58, fill=0.03, elim=(0, 60), ranges=[0, 60], model="hip", psize_seed=48)
    for sol in (merged, _bipartite(200, 9, 3, 6, seed=8), width_solver(300, 70)):
        kf = known_factor_data(sol, 31, dtype)
        dev = to_dev(kf.data)
        with sol.forcePerOp():
            sol.factor(dev)
            kf.check_factor(dev.cpu().numpy(), "per-op")
            for nrhs in (1, 3):
                for op in ("A", "L", "Lt"):
                    _solve(kf, dev, nrhs, op, what="per-op")


# ---- solves -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_rhs_counts(monkeypatch, dtype):
    """nRHS around the groups of 8 and 16, full solves and each triangle, on an elimination range with
    a dense part below and on a wide lump that the sweeps take"""
    monkeypatch.setenv("BSP_SWEEP_MIN_WIDTH", "128")
    for sol in (_bipartite(500, 15, 3, 9, seed=3), width_solver(577, 70)):
        kf, dev = _factor(sol, dtype, 40, "rhs counts")
        for nrhs in (1, 2, 3, 7, 8, 15, 16, 17):
            for op in ("A", "L", "Lt"):
                _solve(kf, dev, nrhs, op, seed=nrhs, what="rhs counts")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mfma", [False, True])
def test_solve_sweeps(monkeypatch, mfma, dtype):
    monkeypatch.setenv("BSP_SWEEP_MIN_WIDTH", "128")
    if mfma:
        monkeypatch.setenv("BSP_SWEEP_MFMA_MIN", "3")
        monkeypatch.setenv("BSP_SWEEP_MFMA_MIN_WIDTH", "0")
    counter = "sweep_mfma_launches" if mfma else "sweep_launches"
    # (the scalar sweep takes up to 16 right-hand sides, the matrix-core one groups of 16)
    for W, tail, nrhs in ((130, 0, 3), (193, 77, 16), (385, 0, 4), (641, 77, 17 if mfma else 11), (1101, 0, 7)):
        sol = width_solver(W, tail)
        kf, dev = _factor(sol, dtype, 5 + W, ("sweep", W))
        for op in ("A", "L", "Lt"):
            took = _counter_delta(sol, counter, lambda: _solve(kf, dev, nrhs, op, what=("sweep", mfma, W)))
            assert took >= 1, (counter, W, op)


SOLVE_SWITCHES = ["solve_wide", "solve_inv", "block_solve", "solve_sweep"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("switch", SOLVE_SWITCHES)
def test_solve_switches(switch, on, dtype):
    """each solve switch on and off, on an elimination range (the wide backward pass from two
    right-hand sides on) and on wide lumps (block solves, inverted diagonal blocks, sweeps)"""
    opts = {switch: on, "sweep_min_width": 128}
    sols = [_bipartite(600, 17, 3, 9, seed=2, hip_options=opts), width_solver(700, 70, hip_options=opts),
            width_solver(1300, 0, hip_options=opts)]
    for sol in sols:
        kf, dev = _factor(sol, dtype, 13, (switch, on))
        for nrhs in (1, 6, 17):
            for op in ("A", "L", "Lt"):
                _solve(kf, dev, nrhs, op, seed=nrhs, what=(switch, on))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_solves(dtype):
    for sol in (_bipartite(300, 11, 3, 9, seed=6), width_solver(400, 70)):
        n, nrhs, bs = sol.order(), 5, 3
        kfs = [known_factor_data(sol, 60 + q, dtype) for q in range(bs)]
        devs = [to_dev(k.data) for k in kfs]
        sol.factor(devs)
        for op, name in (("A", "solve"), ("L", "solveL"), ("Lt", "solveLt")):
            bs_ = [_rhs(n, nrhs, dtype, 70 + q) for q in range(bs)]
            vecs = [to_dev(b.T.ravel().astype(dtype)) for b in bs_]
            getattr(sol, name)(devs, vecs, n, nrhs)
            for q in range(bs):
                kfs[q].check_solve(bs_[q], vec_to_cols(vecs[q].cpu().numpy(), n, nrhs), op, ("batched", q))


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_solves_at_lump_boundaries(dtype):
    """solveLUpTo + solveLFrom is solveL and solveLtFrom + solveLtUpTo is solveLt, at every lump
    boundary beyond the elimination range (and at its end), single and batched"""
    sol = _random_with_range(7)
    sk = sol.skel()
    n, nrhs = sol.order(), 3
    kf, dev = _factor(sol, dtype, 3, "partial")
    first = int(sol.sparseEliminationRanges()[-1])
    assert sol.numLumps() - first >= 5
    b = _rhs(n, nrhs, dtype, 9)
    for lump in range(first + 1, sol.numLumps()):
        span = int(sk["lumpToSpan"][lump])
        v = to_dev(b.T.ravel().astype(dtype))
        sol.solveLUpTo(dev, span, v, n, nrhs)
        sol.solveLFrom(dev, span, v, n, nrhs)
        kf.check_solve(b, vec_to_cols(v.cpu().numpy(), n, nrhs), "L", ("solveL split", lump))
        v = to_dev(b.T.ravel().astype(dtype))
        sol.solveLtFrom(dev, span, v, n, nrhs)
        sol.solveLtUpTo(dev, span, v, n, nrhs)
        kf.check_solve(b, vec_to_cols(v.cpu().numpy(), n, nrhs), "Lt", ("solveLt split", lump))
    span = int(sk["lumpToSpan"][first + 1])
    v = [to_dev(b.T.ravel().astype(dtype))]
    sol.solveLUpTo([dev], span, v, n, nrhs)
    sol.solveLFrom([dev], span, v, n, nrhs)
    kf.check_solve(b, vec_to_cols(v[0].cpu().numpy(), n, nrhs), "L", "batched split")


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_mv_from(dtype):
    """out += alpha A in on the trailing block from span 0, from the end of the elimination range and
    from the last lump, against the product of the data as passed: error over
    |alpha| ||A|| ||in|| + ||out||, worst right-hand side"""
    sol = _random_with_range(12)
    sk = sol.skel()
    n, nrhs, alpha = sol.order(), 3, 0.75
    kf = known_factor_data(sol, 4, dtype)
    dm = to_dev(kf.data)
    first = int(sol.sparseEliminationRanges()[-1])
    vin, vout = _rhs(n, nrhs, dtype, 1), _rhs(n, nrhs, dtype, 2)
    for lump in (0, first, sol.numLumps() - 1):
        span = int(sk["lumpToSpan"][lump])
        bar = int(sk["spanStart"][span])
        di, do = to_dev(vin.T.ravel().astype(dtype)), to_dev(vout.T.ravel().astype(dtype))
        sol.addMvFrom(dm, span, di, n, do, n, nrhs, alpha)
        got = vec_to_cols(do.cpu().numpy(), n, nrhs)
        want = vout.copy()
        Ab = kf.A[bar:, bar:]
        want[bar:] += alpha * (Ab @ vin[bar:])
        scale = alpha * np.linalg.norm(Ab) * np.linalg.norm(vin[bar:], axis=0) + np.linalg.norm(vout, axis=0)
        err = float(np.max(np.linalg.norm(got - want, axis=0) / scale))
        check({"backward": err}, dtype, ("addMvFrom", lump))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pseudo_factor_from(dtype):
    """per-span Cholesky of the diagonal block and division of the rows below, from span 0 and from a
    span beyond the elimination range, against the same computation in float64"""
    sol = _random_with_range(13)
    sk = sol.skel()
    ss = sk["spanStart"]
    kf = known_factor_data(sol, 5, dtype)
    first = int(sol.sparseEliminationRanges()[-1])
    for span0 in (0, int(sk["lumpToSpan"][first]) + 1):
        want = np.tril(kf.A)
        for j in range(span0, sol.numSpans()):
            a, b = int(ss[j]), int(ss[j + 1])
            Ld = np.linalg.cholesky(want[a:b, a:b])
            want[a:b, a:b] = Ld
            want[b:, a:b] = np.linalg.solve(Ld, want[b:, a:b].T).T
        d = to_dev(kf.data)
        sol.pseudoFactorFrom(d, span0)
        got = np.tril(sol.densify(d.cpu().numpy().astype(np.float64)))
        P = stored_pattern(sol)
        lo = int(ss[span0])
        region = np.zeros_like(P)
        region[:, lo:] = True
        region &= P
        ref = want[region]
        err = float(np.linalg.norm(got[region] - ref) / np.linalg.norm(ref))
        check({"off": err}, dtype, ("pseudoFactorFrom", span0))
        # (columns before span0 are left as they were)
        keep = P & ~region
        assert np.array_equal(got[keep], np.tril(kf.A)[keep])
