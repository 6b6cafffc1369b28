"""GPU: partial factorization (factorUpTo / factorFrom / doElimination) on known-factor data
(tests/known_factor.py) at tolerances scaled to the working precision.

factorUpTo(k) runs a plan of its own for the lumps before k, whose board segments also write the
cross-cut updates that leave the Schur complement S = A22 - L21 L21^T in the trailing block; factorFrom
(k) a plan for the lumps from k on.  Each split is checked on the leading columns and on S (with the
trailing entries that no cross-cut product reaches bitwise unchanged), factorFrom on top of it against
the full factor and one solve, and factorFrom alone on data whose leading columns are NaN against the
Cholesky factor of A22.  The structures take the plan's range-dependent paths: the persistent tail,
lookahead, split-K, folded potrf, batches and sub-batches, one wide camera lump fed by the MFMA gather,
elimination ranges and incomplete fill; the run counters assert that each switched path was taken."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from helpers import to_dev
from kf_structures import (affine_plane_cameras, bipartite, blocks_over_separator, counter_delta,
                           lump_over_lump, random_with_range)
from known_factor import bitwise_equal, known_factor_data, leading_words, tolerance, vec_to_cols

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
MAX_SPLITS = 30


def _rhs(n, nrhs, dtype, seed):
    return np.random.default_rng(seed).standard_normal((n, nrhs)).astype(dtype).astype(np.float64)


def _bar(sol, span):
    return int(sol.skel()["spanStart"][span])


def _span_of_lump(sol, lump):
    return int(sol.skel()["lumpToSpan"][lump])


def admissible_splits(sol, seed=0):
    """spans at which factorUpTo / factorFrom may split: every lump boundary from the end of the last
    elimination range on, every elimination-range boundary, 0 and numSpans(), up to
    canFactorUpToSpan().  More than MAX_SPLITS: a seeded sample that keeps 0, numSpans() and the
    boundaries next to the ranges"""
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    dense_from = ranges[-1] if ranges else 0
    lumps = set(range(dense_from, sol.numLumps() + 1)) | set(ranges) | {0}
    lim = sol.canFactorUpToSpan()
    spans = sorted({_span_of_lump(sol, l) for l in lumps if _span_of_lump(sol, l) <= lim})
    if len(spans) <= MAX_SPLITS:
        return spans
    keep = {_span_of_lump(sol, l) for l in set(ranges) | {0, dense_from + 1, sol.numLumps()}
            if l <= sol.numLumps()}
    keep = {s for s in keep if s <= lim}
    rest = sorted(set(spans) - keep)
    pick = np.random.default_rng(seed).choice(len(rest), size=MAX_SPLITS - len(keep), replace=False)
    return sorted(keep | {rest[i] for i in pick})


def _full_factor(sol, kf):
    dev = to_dev(kf.data)
    sol.factor(dev)
    return dev.cpu().numpy()


def _same_as_factor(sol, kf, got, ref, what):
    """`got` comes from the plan that factor() runs: bitwise its result, unless factor() itself is not
    reproducible bitwise (atomic accumulation); then the known-factor check"""
    if bitwise_equal(got, ref):
        return
    assert not bitwise_equal(_full_factor(sol, kf), ref), ("differs from factor() bitwise", what)
    kf.check_factor(got, what)


def _solve_check(kf, dev, nrhs, seed, what):
    sol, n, dtype = kf.sol, kf.sol.order(), kf.dtype
    b = _rhs(n, nrhs, dtype, seed)
    v = to_dev(b.T.ravel().astype(dtype))
    sol.solve(dev, v, n, nrhs)
    kf.check_solve(b, vec_to_cols(v.cpu().numpy(), n, nrhs), "A", what)


def _from_on_nan_leading(sol, kf, span, what):
    """factorFrom(span) alone on data whose leading columns are NaN: it neither reads nor writes them"""
    bar = _bar(sol, span)
    end = leading_words(sol, span)
    data = kf.data.copy()
    data[:end] = np.nan
    dev = to_dev(data)
    sol.factorFrom(dev, span)
    got = dev.cpu().numpy()
    assert bitwise_equal(got[:end], data[:end]), ("factorFrom wrote a leading word", span, what)
    if bar < sol.order():
        kf.check_trailing_factor(got, bar, ("factorFrom on NaN leading columns", span, what))


def check_split(sol, kf, span, what, ref=None):
    """factorUpTo(span); then factorFrom(span); and factorFrom(span) alone on NaN leading columns"""
    bar = _bar(sol, span)
    dev = to_dev(kf.data)
    sol.factorUpTo(dev, span)
    got = dev.cpu().numpy()
    kf.check_partial(got, bar, ("factorUpTo", span, what))
    if span == 0:
        assert bitwise_equal(got, kf.data), ("factorUpTo(0) changed the data", what)
    if span == sol.numSpans() and ref is not None:
        _same_as_factor(sol, kf, got, ref, ("factorUpTo(numSpans)", what))
    sol.factorFrom(dev, span)
    got = dev.cpu().numpy()
    kf.check_factor(got, ("factorUpTo + factorFrom", span, what))
    _solve_check(kf, dev, 2, span, ("after factorFrom", span, what))
    if span == 0 and ref is not None:
        _same_as_factor(sol, kf, got, ref, ("factorFrom(0)", what))
    _from_on_nan_leading(sol, kf, span, what)


def _all_splits(sol, dtype, seed, what):
    kf = known_factor_data(sol, seed, dtype)
    ref = _full_factor(sol, kf)
    kf.check_factor(ref, ("factor", what))
    splits = admissible_splits(sol, seed)
    assert splits[0] == 0 and splits[-1] == sol.numSpans(), splits
    for span in splits:
        check_split(sol, kf, span, what, ref)


# ---- every admissible split -------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_random_structure_every_split(dtype):
    sol = random_with_range(7)
    assert sol.numLumps() - int(sol.sparseEliminationRanges()[-1]) >= 5
    _all_splits(sol, dtype, 3, "random_with_range")


def _ranges_solver():
    """points cut into three given elimination ranges, 6-wide cameras behind them"""
    sol = bipartite(300, 13, 3, 6, seed=5, ranges=[0, 100, 200, 300])
    assert len(sol.sparseEliminationRanges()) >= 4, sol.sparseEliminationRanges()
    return sol


@pytest.mark.parametrize("dtype", DTYPES)
def test_elimination_ranges_every_split(dtype):
    _all_splits(_ranges_solver(), dtype, 4, "bipartite, three ranges")


@pytest.mark.parametrize("dtype", DTYPES)
def test_chained_do_elimination(dtype):
    """doElimination(0), (1), ... on one buffer is factorUpTo at each range end"""
    sol = _ranges_solver()
    kf = known_factor_data(sol, 6, dtype)
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    dev = to_dev(kf.data)
    for r in range(len(ranges) - 1):
        sol.doElimination(dev, r)
        kf.check_partial(dev.cpu().numpy(), int(sol.skel()["lumpStart"][ranges[r + 1]]), ("doElimination", r))


# ---- the dense phase's range-dependent paths --------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_lump_over_narrow_lookahead(dtype):
    """a 1100-wide lump over a 70-wide one, split between them: the factorUpTo plan has lookahead units
    on the side stream, and the Schur complement is read back right after the call"""
    sol = lump_over_lump(1100, 70, hip_options={"tail_blocks": 0})
    kf = known_factor_data(sol, 8, dtype)
    span = _span_of_lump(sol, 1)
    dev = to_dev(kf.data)
    forks = counter_delta(sol, "lookahead_forks", lambda: sol.factorUpTo(dev, span))
    got = dev.cpu().numpy()  # (no synchronize in between)
    assert forks > 0, forks
    kf.check_partial(got, _bar(sol, span), "lookahead")
    sol.factorFrom(dev, span)
    kf.check_factor(dev.cpu().numpy(), "lookahead, factorFrom")
    _solve_check(kf, dev, 3, 1, "lookahead")


# (root width, tail option when on): wide roots take 4 outer blocks of tail, narrow ones the default
ROOTS = [(1599, 4), (2049, 4), (640, -1), (990, -1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tail", ["on", "off"])
@pytest.mark.parametrize("root", ROOTS, ids=lambda r: "W%d" % r[0])
def test_lump_above_root_tail(root, tail, dtype):
    """a 100-wide lump above the root lump, split at the root: factorUpTo leaves S in the root,
    factorFrom factors it with the persistent tail on or off; batched, factorFrom runs the plan without
    the tail (the tag-2 plan)"""
    W, blocks = root
    opts = {"tail_blocks": 0} if tail == "off" else ({"tail_blocks": blocks} if blocks > 0 else None)
    sol = lump_over_lump(100, W, below_span=8 if W % 2 == 0 else 7, hip_options=opts)
    span = _span_of_lump(sol, 1)
    bar = _bar(sol, span)
    kf = known_factor_data(sol, 3 + W, dtype)
    dev = to_dev(kf.data)
    sol.factorUpTo(dev, span)
    kf.check_partial(dev.cpu().numpy(), bar, ("root", W, tail))
    took = counter_delta(sol, "tail_launches", lambda: sol.factorFrom(dev, span))
    assert took == (1 if tail == "on" else 0), (W, tail, took)
    kf.check_factor(dev.cpu().numpy(), ("root", W, tail))
    _solve_check(kf, dev, 2, W, ("root", W, tail))
    _from_on_nan_leading(sol, kf, span, ("root", W, tail))
    kfs = [kf] + [known_factor_data(sol, 50 + W + q, dtype) for q in range(2)]
    devs = [to_dev(k.data) for k in kfs]
    sol.factorUpTo(devs, span)
    for q, (k, d) in enumerate(zip(kfs, devs)):
        k.check_partial(d.cpu().numpy(), bar, ("root batched", W, tail, q))
    took = counter_delta(sol, "tail_launches", lambda: sol.factorFrom(devs, span))
    assert took == 0, (W, tail, took)
    for q, (k, d) in enumerate(zip(kfs, devs)):
        k.check_factor(d.cpu().numpy(), ("root batched", W, tail, q))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("switch", [("BSP_SPLIT_K", "split_lists_used"), ("BSP_POTRF_IN_TRSM", "potrf_folded_levels")],
                         ids=lambda s: s[0])
@pytest.mark.parametrize("on", ["1", "0"])
def test_blocks_over_separator_split(monkeypatch, switch, on, dtype):
    """independent blocks over a separator, split at the root lump (the separator with the block that
    the ordering puts last): the other blocks' levels of several panels (split-K lists, potrf folded
    into the trsm launch) write the cross-cut updates"""
    env, counter = switch
    monkeypatch.setenv(env, on)
    widths = [130, 130, 200, 200] if env == "BSP_SPLIT_K" else [130, 97, 200, 70]
    sol = blocks_over_separator(widths, 150)
    assert sol.numLumps() == len(widths)
    span = _span_of_lump(sol, sol.numLumps() - 1)
    for bs in (1, 3):
        kfs = [known_factor_data(sol, 70 + q, dtype) for q in range(bs)]
        devs = [to_dev(k.data) for k in kfs]
        used = counter_delta(sol, counter, lambda: sol.factorUpTo(devs if bs > 1 else devs[0], span))
        assert (used > 0) == (on == "1"), (env, on, used)
        for q, (k, d) in enumerate(zip(kfs, devs)):
            k.check_partial(d.cpu().numpy(), _bar(sol, span), (env, on, bs, q))
        sol.factorFrom(devs if bs > 1 else devs[0], span)
        for q, (k, d) in enumerate(zip(kfs, devs)):
            k.check_factor(d.cpu().numpy(), (env, on, bs, q))


# ---- one wide camera lump behind the MFMA gather ------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_camera_lump_full_factor(dtype):
    """121 cameras of 16: one dense lump of 8 outer blocks, every target block one of more than 4096
    MFMA gather items"""
    sol = affine_plane_cameras(11, 3, 16)
    assert sol.numLumps() == int(sol.sparseEliminationRanges()[-1]) + 1
    kf = known_factor_data(sol, 12, dtype)
    dev = to_dev(kf.data)
    sol.factor(dev)
    kf.check_factor(dev.cpu().numpy(), "camera lump, factor")
    _solve_check(kf, dev, 2, 3, "camera lump")


@pytest.mark.parametrize("dtype", DTYPES)
def test_camera_lump_up_to_and_from(dtype):
    """the same cameras with dense lumps behind them: the full factor, then factorUpTo(camera lump + 1),
    whose plan ends with the camera lump, and factorFrom on top of it"""
    sol = affine_plane_cameras(11, 3, 16, extra=10)
    cams = int(sol.sparseEliminationRanges()[-1])
    assert sol.numLumps() >= cams + 2
    span = _span_of_lump(sol, cams + 1)
    kf = known_factor_data(sol, 13, dtype)
    dev = to_dev(kf.data)
    sol.factor(dev)
    kf.check_factor(dev.cpu().numpy(), "camera lump and trailing lumps, factor")
    dev = to_dev(kf.data)
    sol.factorUpTo(dev, span)
    kf.check_partial(dev.cpu().numpy(), _bar(sol, span), "camera lump, factorUpTo")
    sol.factorFrom(dev, span)
    kf.check_factor(dev.cpu().numpy(), "camera lump, factorFrom")


# ---- batches ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [2, 5, 17])
def test_batched_partial(bs, dtype):
    """each member with its own L0, at the end of the elimination range and at a dense split"""
    sol = random_with_range(9)
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    for lump in (ranges[-1], (ranges[-1] + sol.numLumps()) // 2):
        span = _span_of_lump(sol, lump)
        kfs = [known_factor_data(sol, 100 * bs + q, dtype) for q in range(bs)]
        devs = [to_dev(k.data) for k in kfs]
        sol.factorUpTo(devs, span)
        for q, (k, d) in enumerate(zip(kfs, devs)):
            k.check_partial(d.cpu().numpy(), _bar(sol, span), ("batched factorUpTo", bs, lump, q))
        sol.factorFrom(devs, span)
        for q, (k, d) in enumerate(zip(kfs, devs)):
            k.check_factor(d.cpu().numpy(), ("batched factorFrom", bs, lump, q))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_partial_sub_batches(monkeypatch, dtype):
    monkeypatch.setenv("BSP_SUB_BATCH_MIN", "2")
    sol = blocks_over_separator([130, 97, 200, 70], 150)
    span = _span_of_lump(sol, sol.numLumps() - 1)
    bs = 5
    kfs = [known_factor_data(sol, 500 + q, dtype) for q in range(bs)]
    devs = [to_dev(k.data) for k in kfs]
    parts = counter_delta(sol, "sub_batches_enqueued", lambda: sol.factorUpTo(devs, span))
    assert parts >= 2, parts
    for q, (k, d) in enumerate(zip(kfs, devs)):
        k.check_partial(d.cpu().numpy(), _bar(sol, span), ("sub-batch factorUpTo", q))
    parts = counter_delta(sol, "sub_batches_enqueued", lambda: sol.factorFrom(devs, span))
    assert parts >= 2, parts
    for q, (k, d) in enumerate(zip(kfs, devs)):
        k.check_factor(d.cpu().numpy(), ("sub-batch factorFrom", q))


# ---- incomplete fill --------------------------------------------------------------------------

def _incomplete_solver():
    """test_create_solver_policies' structure under AddFillForGivenElims: fill complete only up to the
    given range [0, 90]"""
    cols = T.make_independent_elim_set(T.random_cols(215, 0.03, 57), 0, 150)
    sol = B.create_solver(B.Settings(addFillPolicy=B.AddFillForGivenElims), T.random_vec(215, 2, 3, 47),
                          T.columns_to_structure(cols), [0, 90])
    assert sol.canFactorUpToSpan() < sol.numSpans()
    return sol


@pytest.mark.parametrize("dtype", DTYPES)
def test_incomplete_fill_up_to_limit(dtype):
    """factorUpTo(canFactorUpToSpan()) against the partial reference (L0 full on the leading columns,
    lump-diagonal on the trailing ones)"""
    sol = _incomplete_solver()
    span = sol.canFactorUpToSpan()
    bar = _bar(sol, span)
    for seed in (1, 2):
        kf = known_factor_data(sol, seed, dtype, full_from=bar)
        dev = to_dev(kf.data)
        sol.factorUpTo(dev, span)
        kf.check_partial(dev.cpu().numpy(), bar, ("incomplete fill", seed))


# ---- the Schur flow of the PCG path -----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_schur_flow(dtype):
    """factorUpTo(k), solveLUpTo(k), S solved in float64 from the device's S, solveLtUpTo(k): x against
    A.  The two solves run on a copy whose trailing lump columns are NaN (they must not read them)"""
    sol = random_with_range(11)
    n, nrhs = sol.order(), 3
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    kf = known_factor_data(sol, 21, dtype)
    for lump in (ranges[-1], ranges[-1] + 1, sol.numLumps() - 1):
        span = _span_of_lump(sol, lump)
        bar = _bar(sol, span)
        dev = to_dev(kf.data)
        sol.factorUpTo(dev, span)
        host = dev.cpu().numpy()
        S = sol.densify(host.astype(np.float64), fill_upper_half=True)[bar:, bar:]
        cut = host.copy()
        cut[leading_words(sol, span):] = np.nan
        mat = to_dev(cut)
        b = _rhs(n, nrhs, dtype, lump)
        v = to_dev(b.T.ravel().astype(dtype))
        sol.solveLUpTo(mat, span, v, n, nrhs)
        y = vec_to_cols(v.cpu().numpy(), n, nrhs)
        y[bar:] = np.linalg.solve(S, y[bar:])
        v = to_dev(y.T.ravel().astype(dtype))
        sol.solveLtUpTo(mat, span, v, n, nrhs)
        kf.check_solve(b, vec_to_cols(v.cpu().numpy(), n, nrhs), "A", ("Schur flow", lump))


# ---- refusals ---------------------------------------------------------------------------------

def test_refusals_leave_data_unchanged():
    """a span inside a lump, a span that cuts an elimination range, a span past canFactorUpToSpan():
    factorUpTo / factorFrom raise (single and batched) and leave the data bitwise as it was"""
    sol = _ranges_solver()
    kf = known_factor_data(sol, 2, np.float64)
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    assert ranges[0] < (ranges[0] + ranges[1]) // 2 < ranges[1]
    cut = _span_of_lump(sol, (ranges[0] + ranges[1]) // 2)
    inc = _incomplete_solver()
    kinc = known_factor_data(inc, 3, np.float64, full_from=_bar(inc, inc.canFactorUpToSpan()))
    past = [s for s in range(inc.canFactorUpToSpan() + 1, inc.numSpans() + 1)
            if int(inc.skel()["spanOffsetInLump"][s]) == 0]
    wide = lump_over_lump(100, 70)
    kwide = known_factor_data(wide, 4, np.float64)
    inside = [s for s in range(wide.numSpans()) if int(wide.skel()["spanOffsetInLump"][s]) != 0]
    assert inside and past
    cases = [(sol, kf, "UpTo", cut), (sol, kf, "From", cut), (wide, kwide, "UpTo", inside[0]),
             (wide, kwide, "From", inside[-1]), (inc, kinc, "UpTo", past[0]),
             (inc, kinc, "UpTo", inc.numSpans()), (inc, kinc, "From", inc.canFactorUpToSpan())]
    for s_, k, which, span in cases:
        dev = to_dev(k.data)
        with pytest.raises(Exception):
            getattr(s_, "factor" + which)(dev, span)
        assert bitwise_equal(dev.cpu().numpy(), k.data), (which, span)
        devs = [to_dev(k.data), to_dev(k.data)]
        with pytest.raises(Exception):
            getattr(s_, "factor" + which)(devs, span)
        for d in devs:
            assert bitwise_equal(d.cpu().numpy(), k.data), ("batched", which, span)


# ---- fault injection --------------------------------------------------------------------------

def test_fault_injection_is_flagged_by_schur():
    """_testSetFault(1) drops the sparse-elimination update: the Schur check of factorUpTo(end of the
    elimination ranges) fails by far, and passes once the fault is off"""
    sol = bipartite(120, 7, 3, 6, seed=4)
    kf = known_factor_data(sol, 2, np.float64)
    span = _span_of_lump(sol, int(sol.sparseEliminationRanges()[-1]))
    bar = _bar(sol, span)
    dev = to_dev(kf.data)
    sol._testSetFault(1)
    try:
        sol.factorUpTo(dev, span)
    finally:
        sol._testSetFault(0)
    got = dev.cpu().numpy()
    errs = kf.partial_errors_dense(np.tril(sol.densify(got.astype(np.float64))), bar)
    assert errs["schur"] > 1e6 * tolerance("schur", np.float64), errs
    with pytest.raises(AssertionError):
        kf.check_partial(got, bar)
    dev = to_dev(kf.data)
    sol.factorUpTo(dev, span)
    kf.check_partial(dev.cpu().numpy(), bar)
