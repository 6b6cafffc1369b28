"""GPU: every device entry point on framed, poisoned and offset buffers (tests/buffer_edges.py).

Every buffer handed to the library is a view into a Frame: it starts at an odd element offset from a
512-byte-aligned base (element-aligned, never 16-byte-aligned) and lies between guards of 4096 sentinel
words.  Every strictly-upper diagonal-block element of every matrix operand holds the sentinel NaN on
entry (after a factor they are poisoned again before the factor is used).  Every vector block has
ld = n + 5 and sentinel padding rows (addMvFrom: n + 3 in, n + 7 out).  After the call and one
synchronize: no guard word and no padding row has changed, and the operands the interface declares
read-only are bitwise what they were.

Values: factor and solves by the known-factor checks of known_factor.py, unchanged, against the
reference of the clean data; the deterministic extensions bitwise against the same call on plain,
unpoisoned, torch-allocated clones.  The run counters assert that the path under test was taken.
tests/test_buffer_edges_cpu.py shows that the references stay inside this contract and that these
checks fail on the mistakes they are there for."""
import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import testing as T
from assembly_ref import duplicated, stored_elements
from buffer_edges import (SENTINEL_BITS, Frame, assert_padding_intact, bitwise_equal, clear_upper, framed,
                          is_sentinel, poison_upper, strided, unpack, upper_words)
from chol_adjoint_ref import lbar_random
from helpers import solver_random, to_dev
from kf_structures import bipartite as _bipartite
from kf_structures import blocks_over_separator as _blocks_over_separator
from kf_structures import counter_delta as _counter_delta
from kf_structures import dense_solver as _dense_solver
from kf_structures import lump_over_lump as _lump_over_lump
from kf_structures import random_with_range as _random_with_range
from known_factor import check, known_factor_data, leading_words, stored_pattern
from partial_adjoint_ref import bar_of, splits
from selinv_cases import build_case
from stress_cases import width_solver

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SOLVES = {"A": "solve", "L": "solveL", "Lt": "solveLt"}
PAD = 5


def _sync():
    torch.cuda.synchronize()


def _rhs(n, nrhs, dtype, seed):
    """n x nRHS right-hand sides, exactly representable in `dtype`"""
    return np.random.default_rng(seed).standard_normal((n, nrhs)).astype(dtype).astype(np.float64)


def _mat_frame(sol, datas, dtype):
    """one sealed frame holding a poisoned copy of every matrix"""
    return framed(dtype, [poison_upper(np.array(d, dtype=dtype), sol) for d in datas])


def _arg(fr, batched=None):
    """the payloads of a frame as the library takes them: one tensor, or the list of a batch"""
    batched = len(fr) > 1 if batched is None else batched
    return fr.views() if batched else fr.view(0)


def _repoison(fr, sol):
    """after a factor: the sentinel into the upper elements again, then seal (the factor is an input now)"""
    for v in fr.views():
        poison_upper(v, sol)
    assert all(is_sentinel(fr.host(q))[upper_words(sol)].all() for q in range(len(fr)))
    return fr.seal()


def _factor(sol, kfs, what="", call=None, batched=None):
    """factor() of the known-factor matrices as payloads of one frame; returns the frame, poisoned again"""
    kfs = kfs if isinstance(kfs, (list, tuple)) else [kfs]
    fr = _mat_frame(sol, [k.data for k in kfs], kfs[0].dtype)
    (call or sol.factor)(_arg(fr, batched))
    _sync()
    fr.assert_intact(what=("factor", what))
    for q, k in enumerate(kfs):
        k.check_factor(fr.host(q), ("factor", what, q))
    return _repoison(fr, sol)


def _counted(sol, counter):
    """(call, box): call(d) runs sol.factor(d) and appends the rise of the run counter to box"""
    box = []
    return (lambda d: box.append(_counter_delta(sol, counter, lambda: sol.factor(d)))), box


def _solve(kf, fr, nrhs, op="A", seed=1, what="", q=0):
    """one solve on the (poisoned, sealed) factor in payload q of `fr`, the vector block in a frame of its
    own with ld = n + 5"""
    sol, n, dtype = kf.sol, kf.sol.order(), kf.dtype
    ld = n + PAD
    b = _rhs(n, nrhs, dtype, seed)
    vf = framed(dtype, [strided(b, ld, dtype)])
    getattr(sol, SOLVES[op])(fr.view(q), vf.view(0), ld, nrhs)
    _sync()
    what = (what, op, nrhs)
    fr.assert_intact(read_only=range(len(fr)), what=what)
    vf.assert_intact(what=what)
    x = vf.host(0)
    assert_padding_intact(x, n, ld, nrhs, what)
    kf.check_solve(b, unpack(x, n, ld, nrhs), op, what)


def _all_solves(kf, fr, counts, seed=1, what=""):
    for nrhs in counts:
        for op in SOLVES:
            _solve(kf, fr, nrhs, op, seed + nrhs, what)


# ---- factor: lump widths ------------------------------------------------------------------------

WIDTH_GROUPS = [(1, 3, 4, 5), (16, 17), (63, 64, 65), (129, 193, 257)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("widths", WIDTH_GROUPS, ids=lambda g: "W%d-%d" % (g[0], g[-1]))
def test_lump_widths(widths, dtype):
    for W in widths:
        for tail in (0, 70):
            sol = width_solver(W, tail)
            kf = known_factor_data(sol, 5 + W, dtype)
            fr = _factor(sol, kf, ("W", W, tail))
            _solve(kf, fr, 1, seed=W, what=("W", W, tail))


# ---- factor: schedule variants of the dense phase -------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("root", [(1599, 7, {"tail_blocks": 4}), (640, 8, None)], ids=lambda r: "W%d" % r[0])
def test_persistent_tail(root, dtype):
    W, span, opts = root
    sol = _dense_solver(W, span=span, hip_options=opts)
    kf = known_factor_data(sol, 3 + W, dtype)
    call, took = _counted(sol, "tail_launches")
    fr = _factor(sol, kf, ("tail", W), call=call)
    assert took == [1], (W, took)
    _solve(kf, fr, 2, seed=W, what=("tail", W))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["fold", "split"])
def test_folded_potrf_and_split_k(monkeypatch, variant, dtype):
    env, counter, widths = {"fold": ("BSP_POTRF_IN_TRSM", "potrf_folded_levels", [130, 97, 200, 70]),
                            "split": ("BSP_SPLIT_K", "split_lists_used", [130, 130, 200, 200])}[variant]
    monkeypatch.setenv(env, "1")
    sol = _blocks_over_separator(widths, 150)
    for bs in (1, 3):
        kfs = [known_factor_data(sol, 90 + q, dtype) for q in range(bs)]
        call, used = _counted(sol, counter)
        fr = _factor(sol, kfs, (variant, bs), call=call)
        assert used[0] > 0, (variant, bs, used)
        _solve(kfs[0], fr, 1, what=(variant, bs))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lookahead(dtype):
    """a dense lump of 1700 columns: lookahead units on the side stream, and the direct-to-LDS loads of the
    bulk tiles from a base that is not 16-byte-aligned"""
    n = 1700
    sol = B.create_solver(B.Settings(hipOptions={"tail_blocks": 0}), np.ones(n, dtype=np.int64),
                          T.columns_to_structure([set(range(i, n)) for i in range(n)]))
    kf = known_factor_data(sol, 23, dtype)
    call, forks = _counted(sol, "lookahead_forks")
    _factor(sol, kf, "lookahead", call=call)
    assert forks[0] > 0, forks


# ---- factor: sparse elimination --------------------------------------------------------------------

# (number of points, pt_size, cam_size): the cases of test_known_factor_gpu.py
ELIM_CASES = {"tiny9": (400, 3, 3), "tiny16": (400, 4, 4), "mfma_w6": (300, 6, 9), "mfma_w12": (150, 12, 7),
              "mfma_w20": (100, 20, 6), "chain_w3": (400, 3, 17), "chain_w7": (250, 7, 18)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(ELIM_CASES))
def test_sparse_elimination(case, dtype):
    pts, pt, cam = ELIM_CASES[case]
    sol = _bipartite(pts, 13, pt, cam, seed=pt * 31 + cam)
    assert len(sol.sparseEliminationRanges()) >= 2
    kf = known_factor_data(sol, 17 + pt, dtype)
    fr = _factor(sol, kf, ("elim", case))
    _solve(kf, fr, 1, seed=pt, what=("elim", case))
    _solve(kf, fr, 5, seed=pt, what=("elim", case))


# ---- factor: batches, sub-batches, the per-op path ---------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [2, 17])
def test_batched_factor(bs, dtype):
    """every member a payload of one frame"""
    for sol in (width_solver(300, 70), _bipartite(200, 9, 3, 6, seed=bs)):
        kfs = [known_factor_data(sol, 1000 * bs + q, dtype) for q in range(bs)]
        _factor(sol, kfs, ("batch", bs))


@pytest.mark.parametrize("dtype", DTYPES)
def test_forced_sub_batches(monkeypatch, dtype):
    monkeypatch.setenv("BSP_SUB_BATCH_MIN", "2")
    sol = _blocks_over_separator([130, 97, 200, 70], 150)
    kfs = [known_factor_data(sol, 500 + q, dtype) for q in range(4)]
    call, parts = _counted(sol, "sub_batches_enqueued")
    _factor(sol, kfs, "sub-batch", call=call)
    assert parts[0] >= 2, parts


@pytest.mark.parametrize("dtype", DTYPES)
def test_per_op_path(dtype):
    """factor and solves through the op-by-op loops"""
    merged, _, _ = solver_random(58, fill=0.03, elim=(0, 60), ranges=[0, 60], model="hip", psize_seed=48)
    for sol in (merged, _bipartite(200, 9, 3, 6, seed=8), width_solver(300, 70)):
        kf = known_factor_data(sol, 31, dtype)
        with sol.forcePerOp():
            fr = _factor(sol, kf, "per-op")
            _all_solves(kf, fr, (1, 3), what="per-op")


# ---- partial factors ----------------------------------------------------------------------------

def _check_cut(sol, kf, span, what):
    """factorUpTo(span), then factorFrom(span) on the same payload; and factorFrom(span) alone on data
    whose leading columns hold the sentinel"""
    dtype = kf.dtype
    bar = bar_of(sol, span)
    fr = _mat_frame(sol, [kf.data], dtype)
    sol.factorUpTo(fr.view(0), span)
    _sync()
    fr.assert_intact(what=("factorUpTo", span, what))
    kf.check_partial(fr.host(0), bar, ("factorUpTo", span, what))
    _repoison(fr, sol)
    sol.factorFrom(fr.view(0), span)
    _sync()
    fr.assert_intact(what=("factorFrom", span, what))
    kf.check_factor(fr.host(0), ("factorUpTo + factorFrom", span, what))
    _solve(kf, _repoison(fr, sol), 2, seed=span, what=("after factorFrom", span, what))
    end = leading_words(sol, span)
    data = poison_upper(kf.data.copy(), sol)
    data.view(np.uint64 if dtype == np.float64 else np.uint32)[:end] = SENTINEL_BITS[dtype]
    fr = framed(dtype, [data])
    sol.factorFrom(fr.view(0), span)
    _sync()
    fr.assert_intact(what=("factorFrom alone", span, what))
    got = fr.host(0)
    assert bitwise_equal(got[:end], data[:end]), ("factorFrom wrote a leading word", span, what)
    if bar < sol.order():
        kf.check_trailing_factor(got, bar, ("factorFrom alone", span, what))


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_factor_at_lump_boundaries(dtype):
    sol = _random_with_range(7)
    first = int(sol.sparseEliminationRanges()[-1])
    assert sol.numLumps() - first >= 5
    kf = known_factor_data(sol, 3, dtype)
    for lump in range(first + 1, sol.numLumps()):
        _check_cut(sol, kf, int(sol.skel()["lumpToSpan"][lump]), "random_with_range")


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_factor_between_two_wide_lumps(dtype):
    sol = _lump_over_lump(200, 130)
    _check_cut(sol, known_factor_data(sol, 8, dtype), int(sol.skel()["lumpToSpan"][1]), "lump_over_lump")


@pytest.mark.parametrize("dtype", DTYPES)
def test_pseudo_factor_from(dtype):
    """the computation of test_known_factor_gpu.py::test_pseudo_factor_from, against the same float64 reference"""
    sol = _random_with_range(13)
    sk = sol.skel()
    ss = sk["spanStart"]
    kf = known_factor_data(sol, 5, dtype)
    P = stored_pattern(sol)
    first = int(sol.sparseEliminationRanges()[-1])
    for span0 in (0, int(sk["lumpToSpan"][first]) + 1):
        want = np.tril(kf.A)
        for j in range(span0, sol.numSpans()):
            a, b = int(ss[j]), int(ss[j + 1])
            Ld = np.linalg.cholesky(want[a:b, a:b])
            want[a:b, a:b] = Ld
            want[b:, a:b] = np.linalg.solve(Ld, want[b:, a:b].T).T
        fr = _mat_frame(sol, [kf.data], dtype)
        sol.pseudoFactorFrom(fr.view(0), span0)
        _sync()
        fr.assert_intact(what=("pseudoFactorFrom", span0))
        got = np.tril(sol.densify(fr.host(0).astype(np.float64)))
        region = np.zeros_like(P)
        region[:, int(ss[span0]):] = True
        region &= P
        ref = want[region]
        err = float(np.linalg.norm(got[region] - ref) / np.linalg.norm(ref))
        check({"off": err}, dtype, ("pseudoFactorFrom", span0))
        keep = P & ~region
        assert np.array_equal(got[keep], np.tril(kf.A)[keep])


# ---- solves -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["bipartite", "wide"])
def test_solve_rhs_counts(monkeypatch, which, dtype):
    monkeypatch.setenv("BSP_SWEEP_MIN_WIDTH", "128")
    sol = _bipartite(500, 15, 3, 9, seed=3) if which == "bipartite" else width_solver(577, 70)
    kf = known_factor_data(sol, 40, dtype)
    fr = _factor(sol, kf, "rhs counts")
    _all_solves(kf, fr, (1, 2, 8, 16, 17), what="rhs counts")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mfma", [False, True])
def test_solve_sweeps(monkeypatch, mfma, dtype):
    monkeypatch.setenv("BSP_SWEEP_MIN_WIDTH", "128")
    if mfma:
        monkeypatch.setenv("BSP_SWEEP_MFMA_MIN", "3")
        monkeypatch.setenv("BSP_SWEEP_MFMA_MIN_WIDTH", "0")
    counter = "sweep_mfma_launches" if mfma else "sweep_launches"
    for W, tail, nrhs in ((193, 77, 16), (641, 77, 17 if mfma else 11)):
        sol = width_solver(W, tail)
        kf = known_factor_data(sol, 5 + W, dtype)
        fr = _factor(sol, kf, ("sweep", W))
        for op in SOLVES:
            took = _counter_delta(sol, counter, lambda: _solve(kf, fr, nrhs, op, what=("sweep", mfma, W)))
            assert took >= 1, (counter, W, op)


SOLVE_SWITCHES = ["solve_wide", "solve_inv", "block_solve", "solve_sweep"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("switch", SOLVE_SWITCHES)
def test_solve_switches(switch, on, dtype):
    opts = {switch: on, "sweep_min_width": 128}
    for sol in (_bipartite(600, 17, 3, 9, seed=2, hip_options=opts), width_solver(700, 70, hip_options=opts)):
        kf = known_factor_data(sol, 13, dtype)
        fr = _factor(sol, kf, (switch, on))
        _all_solves(kf, fr, (1, 6, 17), what=(switch, on))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pt_size,cam_size", [(1, 40), (2, 37), (3, 25), (4, 19)])
def test_wide_backward_pass(pt_size, cam_size, dtype):
    """the backward pass over the elimination range with the right-hand sides across the lanes (it copies the
    rows below the range as [16][rows] first): every lump width it is instantiated for, camera blocks taller
    than one pass, a lump count that is no multiple of the 16 per workgroup"""
    sol = _bipartite(1003, 23, pt_size, cam_size, seed=9 + pt_size)
    kf = known_factor_data(sol, 3, dtype)
    fr = _factor(sol, kf, ("wide", pt_size))
    took = _counter_delta(sol, "solve_wide_launches", lambda: _solve(kf, fr, 17, "A", what=("wide", pt_size)))
    assert took == 1, (pt_size, cam_size, took)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_widths_take_the_row_per_lane_kernel(dtype):
    sol = _bipartite(600, 17, 1 + (np.arange(600) % 3), 8, seed=4)
    kf = known_factor_data(sol, 3, dtype)
    fr = _factor(sol, kf, "mixed widths")
    took = _counter_delta(sol, "solve_wide_launches", lambda: _solve(kf, fr, 6, "A", what="mixed widths"))
    assert took == 0, took
    _solve(kf, fr, 6, "Lt", what="mixed widths")


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_solves(dtype):
    """members in one frame, their vector blocks in another"""
    for sol in (_bipartite(300, 11, 3, 9, seed=6), width_solver(400, 70)):
        n, nrhs, bs = sol.order(), 5, 3
        ld = n + PAD
        kfs = [known_factor_data(sol, 60 + q, dtype) for q in range(bs)]
        fr = _factor(sol, kfs, "batched solves")
        for op, name in SOLVES.items():
            bs_ = [_rhs(n, nrhs, dtype, 70 + q) for q in range(bs)]
            vf = framed(dtype, [strided(b, ld, dtype) for b in bs_])
            getattr(sol, name)(fr.views(), vf.views(), ld, nrhs)
            _sync()
            fr.assert_intact(read_only=range(bs), what=("batched", op))
            vf.assert_intact(what=("batched", op))
            for q in range(bs):
                x = vf.host(q)
                assert_padding_intact(x, n, ld, nrhs, ("batched", op, q))
                kfs[q].check_solve(bs_[q], unpack(x, n, ld, nrhs), op, ("batched", op, q))


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_solves_at_lump_boundaries(dtype):
    """solveLUpTo + solveLFrom is solveL and solveLtFrom + solveLtUpTo is solveLt, at every lump boundary
    beyond the elimination range, single and batched"""
    sol = _random_with_range(7)
    sk = sol.skel()
    n, nrhs = sol.order(), 3
    ld = n + PAD
    kf = known_factor_data(sol, 3, dtype)
    fr = _factor(sol, kf, "partial solves")
    first = int(sol.sparseEliminationRanges()[-1])
    assert sol.numLumps() - first >= 5
    b = _rhs(n, nrhs, dtype, 9)

    def run(pair, op, span, batched, what):
        vf = framed(dtype, [strided(b, ld, dtype)])
        for name in pair:
            if batched:
                getattr(sol, name)([fr.view(0)], span, [vf.view(0)], ld, nrhs)
            else:
                getattr(sol, name)(fr.view(0), span, vf.view(0), ld, nrhs)
            _sync()
            fr.assert_intact(read_only=(0,), what=(name, what))
            vf.assert_intact(what=(name, what))
            assert_padding_intact(vf.host(0), n, ld, nrhs, (name, what))
        kf.check_solve(b, unpack(vf.host(0), n, ld, nrhs), op, what)

    for lump in range(first + 1, sol.numLumps()):
        span = int(sk["lumpToSpan"][lump])
        run(("solveLUpTo", "solveLFrom"), "L", span, False, ("solveL split", lump))
        run(("solveLtFrom", "solveLtUpTo"), "Lt", span, False, ("solveLt split", lump))
    span = int(sk["lumpToSpan"][first + 1])
    run(("solveLUpTo", "solveLFrom"), "L", span, True, "batched solveL split")
    run(("solveLtFrom", "solveLtUpTo"), "Lt", span, True, "batched solveLt split")


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_mv_from(dtype):
    """out += alpha A in behind span 0, behind the elimination range and on the last lump, with in_stride
    n + 3 and out_stride n + 7; mat and vec_in are read-only"""
    sol = _random_with_range(12)
    sk = sol.skel()
    n, nrhs, alpha = sol.order(), 3, 0.75
    ldi, ldo = n + 3, n + 7
    kf = known_factor_data(sol, 4, dtype)
    first = int(sol.sparseEliminationRanges()[-1])
    vin, vout = _rhs(n, nrhs, dtype, 1), _rhs(n, nrhs, dtype, 2)
    for lump in (0, first, sol.numLumps() - 1):
        span = int(sk["lumpToSpan"][lump])
        bar = int(sk["spanStart"][span])
        fr = framed(dtype, [poison_upper(kf.data.copy(), sol), strided(vin, ldi, dtype), strided(vout, ldo, dtype)])
        sol.addMvFrom(fr.view(0), span, fr.view(1), ldi, fr.view(2), ldo, nrhs, alpha)
        _sync()
        fr.assert_intact(read_only=(0, 1), what=("addMvFrom", lump))
        out = fr.host(2)
        assert_padding_intact(out, n, ldo, nrhs, ("addMvFrom", lump))
        got = unpack(out, n, ldo, nrhs)
        want = vout.copy()
        Ab = kf.A[bar:, bar:]
        want[bar:] += alpha * (Ab @ vin[bar:])
        scale = alpha * np.linalg.norm(Ab) * np.linalg.norm(vin[bar:], axis=0) + np.linalg.norm(vout, axis=0)
        err = float(np.max(np.linalg.norm(got - want, axis=0) / scale))
        check({"backward": err}, dtype, ("addMvFrom", lump))
        assert bitwise_equal(got[:bar].astype(dtype), vout[:bar].astype(dtype)), ("rows before the block changed", lump)


# ---- extensions: bitwise against the same call on plain, unpoisoned clones -----------------------------

EXT = {"mixed_owners": lambda: build_case("mixed_owners")[0],
       "width129": lambda: build_case("width129")[0],
       "forest": lambda: build_case("forest")[0],
       "random_elim": lambda: solver_random(3, fill=0.037, elim=(0, 60))[0]}
K = 17


def _ext_factors(sol, dtype, nb, seed=5):
    """nb known-factor matrices (rho = 0.5, as the adjoint tests use) factored as one framed batch: the host
    factors, poisoned (what the framed calls get) and with zeros above the diagonal (what the plain calls get)"""
    kfs = [known_factor_data(sol, seed + q, dtype, rho=0.5) for q in range(nb)]
    fr = _factor(sol, kfs, "extensions")
    Ls = [fr.host(q) for q in range(nb)]
    assert all(is_sentinel(L)[upper_words(sol)].all() for L in Ls)
    return kfs, Ls, [clear_upper(L, sol) for L in Ls]


def _same(got, want, what):
    """bitwise, and the plain call's result has no NaN (a poisoned call that matches it has none either)"""
    want = want.cpu().numpy() if hasattr(want, "cpu") else np.asarray(want)
    assert not np.isnan(want).any(), ("the plain call gave NaN", what)
    if not bitwise_equal(np.asarray(got).ravel(), want.ravel()):
        bad = np.asarray(got).ravel() != want.ravel()
        raise AssertionError(("differs from the call on plain clones", what, "%d of %d elements" % (int(bad.sum()), bad.size),
                              "%d NaN" % int(np.isnan(np.asarray(got)).sum()), "first at %d" % int(np.argmax(bad))))


def _plain_cols(M, ld, dtype):
    """[n, k] -> k columns of stride ld with zero padding, on the device (a plain allocation)"""
    out = np.zeros((M.shape[1], ld), dtype=dtype)
    out[:, :M.shape[0]] = M.T
    return to_dev(out.ravel())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(EXT))
def test_selected_inverse_and_log_det(name, dtype):
    sol = EXT[name]()
    _, Lp, Lc = _ext_factors(sol, dtype, 5)
    plain = []
    for L in Lc:
        z = to_dev(L)
        sol.selectedInverse(z)
        plain.append(z)
    # single
    fr = framed(dtype, [Lp[0]])
    sol.selectedInverse(fr.view(0))
    _sync()
    fr.assert_intact(what="selectedInverse")
    _same(fr.host(0), plain[0], "selectedInverse")
    # a batch of 5 in one frame
    fr = framed(dtype, Lp)
    sol.selectedInverse(fr.views())
    _sync()
    fr.assert_intact(what="selectedInverse, batch")
    for q in range(5):
        _same(fr.host(q), plain[q], ("selectedInverse, batch", q))
    # logDet
    fr = framed(dtype, [Lp[0]])
    got = sol.logDet(fr.view(0))
    _sync()
    fr.assert_intact(read_only=(0,), what="logDet")
    _same(got.cpu().numpy(), sol.logDet(to_dev(Lc[0])), "logDet")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(EXT))
def test_pattern_grad_and_outer(name, dtype):
    sol = EXT[name]()
    n, ds = sol.order(), sol.dataSize()
    ld = n + PAD
    rng = np.random.default_rng(3)
    U, V = rng.uniform(-1, 1, (n, K)).astype(dtype), rng.uniform(-1, 1, (n, K)).astype(dtype)
    Z = rng.uniform(-1, 1, ds).astype(dtype)
    s = np.array([0.75], dtype=dtype)
    Up, Vp, Zc, sp = _plain_cols(U, ld, dtype), _plain_cols(V, ld, dtype), to_dev(clear_upper(Z, sol)), to_dev(s)
    tdt = Up.dtype

    def frame():
        # payloads: out (left full of the sentinel: it is never read), Z, zScale, U, V
        fr = Frame([ds, ds, 1, K * ld, K * ld], dtype)
        for k, a in ((1, poison_upper(Z.copy(), sol)), (2, s), (3, strided(U, ld, dtype)), (4, strided(V, ld, dtype))):
            fr.fill(k, a)
        return fr.seal()

    def plain_out():
        return torch.full((ds,), float("nan"), dtype=tdt, device="cuda")

    cases = [("patternGrad Z", lambda o, z, sc, u, v: sol.patternGrad(o, Z=z, zScale=sc)),
             ("patternGrad U V", lambda o, z, sc, u, v: sol.patternGrad(o, U=u, V=v, nRHS=K, alpha=-1.5, stride=ld)),
             ("patternGrad Z U V", lambda o, z, sc, u, v: sol.patternGrad(o, Z=z, zScale=sc, U=u, V=v, nRHS=K, alpha=-1.5,
                                                                         stride=ld)),
             ("patternOuter", lambda o, z, sc, u, v: sol.patternOuter(o, u, v, nRHS=K, alpha=-0.5, stride=ld))]
    for what, call in cases:
        fr = frame()
        call(*fr.views())
        _sync()
        fr.assert_intact(read_only=(1, 2, 3, 4), what=what)
        want = plain_out()
        call(want, Zc, sp, Up, Vp)
        _same(fr.host(0), want, what)
        assert (fr.host(0)[upper_words(sol)] == 0).all(), what


def _interior_cut(sol):
    sp = splits(sol)
    span = sp[len(sp) // 2]
    assert 0 < span < sol.numSpans()
    return span


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(EXT))
def test_factor_adjoint(name, dtype):
    sol = EXT[name]()
    _, Lp, Lc = _ext_factors(sol, dtype, 5)
    lbars = [lbar_random(sol, 100 + q, dtype) for q in range(5)]
    plain = []
    for L, lb in zip(Lc, lbars):
        g = to_dev(lb)
        sol.factorAdjoint(to_dev(L), g)
        plain.append(g)
    fr = framed(dtype, [Lp[0], poison_upper(lbars[0].copy(), sol)])
    sol.factorAdjoint(fr.view(0), fr.view(1))
    _sync()
    fr.assert_intact(read_only=(0,), what="factorAdjoint")
    _same(fr.host(1), plain[0], "factorAdjoint")
    fr = framed(dtype, Lp + [poison_upper(lb.copy(), sol) for lb in lbars])
    sol.factorAdjoint(fr.views()[:5], fr.views()[5:])
    _sync()
    fr.assert_intact(read_only=range(5), what="factorAdjoint, batch")
    for q in range(5):
        _same(fr.host(5 + q), plain[q], ("factorAdjoint, batch", q))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(EXT))
def test_partial_adjoint_and_schur_complement(name, dtype):
    sol = EXT[name]()
    span = _interior_cut(sol)
    bar = bar_of(sol, span)
    m, ds = sol.order() - bar, sol.dataSize()
    kf = known_factor_data(sol, 5, dtype, rho=0.5)
    fr = _mat_frame(sol, [kf.data], dtype)
    sol.factorUpTo(fr.view(0), span)
    _sync()
    fr.assert_intact(what="factorUpTo")
    kf.check_partial(fr.host(0), bar, ("factorUpTo", name))
    Pp = poison_upper(fr.host(0), sol)
    Pc = to_dev(clear_upper(Pp, sol))
    # factorAdjointUpTo
    pbar = lbar_random(sol, 22 + span, dtype)
    want = to_dev(pbar)
    sol.factorAdjointUpTo(Pc, want, span)
    fr = framed(dtype, [Pp, poison_upper(pbar.copy(), sol)])
    sol.factorAdjointUpTo(fr.view(0), fr.view(1), span)
    _sync()
    fr.assert_intact(read_only=(0,), what="factorAdjointUpTo")
    _same(fr.host(1), want, "factorAdjointUpTo")
    # schurComplement: the dense output is a payload too
    fr = Frame([ds, m * m], dtype).fill(0, Pp).seal()
    ret = sol.schurComplement(fr.view(0), span, out=fr.view(1).view(m, m))
    _sync()
    assert ret.data_ptr() == fr.view(1).data_ptr()
    fr.assert_intact(read_only=(0,), what="schurComplement")
    S = sol.schurComplement(Pc, span)
    _same(fr.host(1), S, "schurComplement")
    assert np.array_equal(S.cpu().numpy(), S.cpu().numpy().T)
    # schurComplementAdjoint
    Gd = np.random.default_rng(span + 1).uniform(-1, 1, (m, m)).astype(dtype)
    fr = Frame([m * m, ds], dtype).fill(0, Gd).seal()
    sol.schurComplementAdjoint(fr.view(0).view(m, m), span, out=fr.view(1))
    _sync()
    fr.assert_intact(read_only=(0,), what="schurComplementAdjoint")
    _same(fr.host(1), sol.schurComplementAdjoint(to_dev(Gd), span), "schurComplementAdjoint")


def _jacobian_on(sol, rng, max_rows=20000):
    """a Jacobian whose J^T J lies on the solver's pattern: one row per stored lower element (i, j), with
    entries in the columns i and j (one entry on the diagonal), in the caller's order, shuffled"""
    r, c = stored_elements(sol)
    if len(r) > max_rows:
        pick = np.sort(rng.choice(len(r), max_rows, replace=False))
        r, c = r[pick], c[pick]
    k = np.arange(len(r), dtype=np.int64)
    off = r != c
    rows, cols = np.concatenate([k, k[off]]), np.concatenate([r, c[off]])
    order = rng.permutation(len(rows))
    return rows[order], cols[order], len(r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(EXT))
def test_assembly_and_normal_equations(name, dtype):
    sol = EXT[name]()
    n, ds = sol.order(), sol.dataSize()
    rng = np.random.default_rng(11)
    gd = [poison_upper(rng.uniform(-1, 1, ds).astype(dtype), sol) for _ in range(3)]

    def cleared(h):
        out = h.copy().reshape(-1, ds)
        out[:, upper_words(sol)] = 0
        return out.reshape(h.shape)

    def run(what, call, ins, out_shape, read_upper=()):
        """call(*inputs, out) single and as a batch of 3 with every tensor a payload, against the same call on
        plain tensors; `ins`: per input the three host members [.., shape]"""
        for nb in (1, 3):
            lead = (nb,) if nb > 1 else ()
            hosts = [np.stack(x[:nb]) if nb > 1 else x[0] for x in ins]
            fr = Frame([h.size for h in hosts] + [nb * int(np.prod(out_shape))], dtype)
            for k, h in enumerate(hosts):
                fr.fill(k, h)
            fr.seal()
            args = [fr.view(k).view(h.shape) for k, h in enumerate(hosts)]
            out = fr.view(len(hosts)).view(lead + tuple(out_shape))
            ret = call(*args, out)
            _sync()
            assert ret.data_ptr() == out.data_ptr()
            fr.assert_intact(read_only=range(len(hosts)), what=(what, nb))
            plain = [to_dev(cleared(h) if k in read_upper else h) for k, h in enumerate(hosts)]
            want = call(*plain, None)
            _same(fr.host(len(hosts)), want, (what, nb))

    # assembly
    rows, cols, _ = duplicated(*stored_elements(sol), rng)
    asm = sol.assembly(rows, cols)
    vals = [rng.uniform(-1, 1, len(rows)).astype(dtype) for _ in range(3)]
    run("Assembly.assemble", lambda v, o: asm.assemble(v, out=o), [vals], (ds,))
    run("Assembly.adjoint", lambda g, o: asm.adjoint(g, out=o), [gd], (len(rows),), read_upper=(0,))
    # normal equations
    jr, jc, m = _jacobian_on(sol, rng)
    ne = sol.normalEquations(jr, jc, m)
    jv = [rng.uniform(-1, 1, len(jr)).astype(dtype) for _ in range(3)]
    q = 3
    r = [rng.uniform(-1, 1, (m, q)).astype(dtype) for _ in range(3)]
    v = [rng.uniform(-1, 1, (n, q)).astype(dtype) for _ in range(3)]
    run("NormalEquations.hessian", lambda a, o: ne.hessian(a, out=o), [jv], (ds,))
    run("NormalEquations.hessianAdjoint", lambda a, g, o: ne.hessianAdjoint(a, g, out=o), [jv, gd], (len(jr),),
        read_upper=(1,))
    run("NormalEquations.jtVec", lambda a, x, o: ne.jtVec(a, x, out=o), [jv, r], (n, q))
    run("NormalEquations.jVec", lambda a, x, o: ne.jVec(a, x, out=o), [jv, v], (m, q))
