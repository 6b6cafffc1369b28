"""GPU: Solver.factorAdjointUpTo (the reverse-mode sweep of factorUpTo()) against
the dense oracle of partial_adjoint_ref.py, and Solver.schurComplement / schurComplementAdjoint against
densify / project.

Data and bounds as test_chol_adjoint_gpu.py: known-factor matrices (rho = 0.5, cond(A) < 100 asserted),
random Pbar with values on the strictly-upper elements too; relative to max |grad| 1e-10 in fp64 and
1e-4 in fp32 (fp32 against the oracle of the fp32-rounded data), set from cond(A) eps before any GPU
run."""
import ctypes

import numpy as np
import pytest
import torch

import baspacho_amd as B
from autograd_ref import element_coords, project
from chol_adjoint_ref import lbar_random, rel_error
from helpers import solver_random, to_dev
from kf_structures import bipartite, blocks_over_separator, lump_over_lump
from known_factor import known_factor_data
from partial_adjoint_ref import bar_of, oracle, splits
from selinv_cases import build_case, case_names

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
TDT = {np.float64: torch.float64, np.float32: torch.float32}


def _data(sol, seed, dtype):
    kf = known_factor_data(sol, seed, dtype, rho=0.5)
    assert np.linalg.cond(kf.A) < 100
    return kf.data


def _partial(sol, data, span):
    P = to_dev(data)
    sol.factorUpTo(P, span)
    return P


def _adjoint(sol, P, pbar, span):
    g = pbar.clone()
    sol.factorAdjointUpTo(P, g, span)
    return g


def _check_splits(sol, seed, dtype, what, spans=None):
    data = _data(sol, seed, dtype)
    coords = element_coords(sol)
    i, j = coords
    for span in (spans if spans is not None else splits(sol)):
        pbar = lbar_random(sol, seed + 17 + span, dtype)
        P = _partial(sol, data, span)
        P0 = P.clone()
        g = _adjoint(sol, P, to_dev(pbar), span)
        g2 = _adjoint(sol, P, to_dev(pbar), span)
        torch.cuda.synchronize()
        assert torch.equal(P, P0), "factorAdjointUpTo wrote to P"
        assert torch.equal(g, g2), "two runs differ"
        got = g.cpu().numpy()
        want, _ = oracle(sol, data, pbar, span, coords)
        err = rel_error(got, want)
        print("%s span %d / %d: %.2e" % (what, span, sol.numSpans(), err))
        assert np.isfinite(got).all() and err < TOL[dtype], (what, span, err)
        assert (got[i < j] == 0).all()
        if span == 0:
            assert np.array_equal(got, np.where(i >= j, pbar, 0).astype(dtype))
        if span == sol.numSpans():
            full = to_dev(pbar)
            sol.factorAdjoint(P, full)
            assert torch.equal(full, g), "span = numSpans() is not factorAdjoint"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", case_names())
def test_selinv_cases_every_split(name, dtype):
    sol, _ = build_case(name)
    _check_splits(sol, 5, dtype, name)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seed", [3, 8])
def test_random_structures_with_elimination_ranges_every_split(seed, dtype):
    sol, _, _ = solver_random(seed, fill=0.037, elim=(0, 60))
    assert len(sol.sparseEliminationRanges()) >= 2
    _check_splits(sol, seed, dtype, "random%d" % seed)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_lumps_on_both_sides_of_the_cut(dtype):
    """nodes (not small lumps) before and behind the cut"""
    sol = lump_over_lump(1100, 70)
    assert sol.numLumps() == 2
    span = int(sol.skel()["lumpToSpan"][1])
    plan = sol._testSelInvPlan(span)
    assert len(plan["node"]["lump"]) > 1 and len(plan["small"]["lump"]) == 0
    _check_splits(sol, 3, dtype, "lump_over_lump", spans=[span])
    sol = blocks_over_separator([150, 90, 200], 130)
    root = int(sol.skel()["lumpToSpan"][sol.numLumps() - 1])
    assert len(sol._testSelInvPlan(root)["node"]["lump"]) > 1
    _check_splits(sol, 4, dtype, "blocks_over_separator", spans=[root])


def _mid_span(sol):
    sp = splits(sol)
    return sp[len(sp) // 2]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_members_are_bitwise_the_single_call(dtype):
    sol, _ = build_case("mixed_owners")
    span = _mid_span(sol)
    assert 0 < span < sol.numSpans()
    P = _partial(sol, _data(sol, 2, dtype), span)
    for B_ in (1, 2, 5, 17):
        pbars = [to_dev(lbar_random(sol, 100 + q, dtype)) for q in range(B_)]
        Ps = [P.clone() for _ in range(B_)]
        single = [_adjoint(sol, P, pb, span) for pb in pbars]
        gs = [pb.clone() for pb in pbars]
        sol.factorAdjointUpTo(Ps, gs, span)
        torch.cuda.synchronize()
        for q in range(B_):
            assert torch.equal(gs[q], single[q]), (B_, q)
            assert torch.equal(Ps[q], P)


def test_batch_in_chunks_is_bitwise_the_single_call():
    sol = lump_over_lump(300, 70)
    span = int(sol.skel()["lumpToSpan"][1])
    P = _partial(sol, _data(sol, 4, np.float64), span)
    pbars = [to_dev(lbar_random(sol, 7 + q)) for q in range(5)]
    single = [_adjoint(sol, P, pb, span) for pb in pbars]
    sol._testSetSelInvBatchChunk(2)
    try:
        gs = [pb.clone() for pb in pbars]
        sol.factorAdjointUpTo([P] * 5, gs, span)
    finally:
        sol._testSetSelInvBatchChunk(0)
    torch.cuda.synchronize()
    for q in range(5):
        assert torch.equal(gs[q], single[q]), q


def test_complete_sweep_is_unchanged_after_partial_sweeps():
    """plans of several cuts share the scratch with the complete plan: factorAdjoint and selectedInverse
    give the same bits before and after"""
    sol, _ = build_case("mixed_owners")
    data = _data(sol, 2, np.float64)
    L = to_dev(data)
    sol.factor(L)
    lbar = to_dev(lbar_random(sol, 3))
    before = lbar.clone()
    sol.factorAdjoint(L, before)
    Z0 = L.clone()
    sol.selectedInverse(Z0)
    for span in splits(sol):
        _adjoint(sol, _partial(sol, data, span), lbar, span)
    after = lbar.clone()
    sol.factorAdjoint(L, after)
    Z1 = L.clone()
    sol.selectedInverse(Z1)
    assert torch.equal(before, after) and torch.equal(Z0, Z1)


def test_refusals_leave_grad_unchanged():
    sol = bipartite(300, 13, 3, 6, seed=5, ranges=[0, 100, 200, 300])
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    cut = int(sol.skel()["lumpToSpan"][(ranges[0] + ranges[1]) // 2])
    wide = lump_over_lump(100, 70)
    inside = [s for s in range(wide.numSpans()) if int(wide.skel()["spanOffsetInLump"][s]) != 0]
    inc, _, _ = solver_random(61, fill=0.03, elim=(0, 60), ranges=[0, 60], policy=B.AddFillForGivenElims)
    assert inc.canFactorUpToSpan() < inc.numSpans() and inside
    cases = [(sol, cut, "sparse-elimination"), (wide, inside[0], "inside a lump"), (wide, -1, "not in"),
             (wide, wide.numSpans() + 1, "not in"), (inc, inc.canFactorUpToSpan(), "complete factor"),
             (inc, 0, "complete factor")]
    for s_, span, msg in cases:
        P = torch.ones(s_.dataSize(), dtype=torch.float64, device="cuda")
        g0 = to_dev(lbar_random(s_, 1))
        g = g0.clone()
        with pytest.raises(RuntimeError, match=msg):
            s_.factorAdjointUpTo(P, g, span)
        gs = [g0.clone(), g0.clone()]
        with pytest.raises(RuntimeError, match=msg):
            s_.factorAdjointUpTo([P, P.clone()], gs, span)
        torch.cuda.synchronize()
        for t in [g] + gs:
            assert torch.equal(t, g0), (span, msg)
    # pointers: NULL, overlap, empty batch
    lib, h, ds = wide._lib, wide._h, wide.dataSize()
    P = torch.ones(ds, dtype=torch.float64, device="cuda")
    g = torch.zeros(2 * ds, dtype=torch.float64, device="cuda")
    p, sp = ctypes.c_void_p, ctypes.c_int64(int(wide.skel()["lumpToSpan"][1]))
    err = lambda: B._lib.load().bsp_last_error().decode()
    for fn in (lib.bsp_factor_adjoint_up_to_f64, lib.bsp_factor_adjoint_up_to_f32):
        assert fn(h, p(None), p(g.data_ptr()), sp) != 0
        assert fn(h, p(P.data_ptr()), p(None), sp) != 0
        assert fn(h, p(P.data_ptr()), p(P.data_ptr()), sp) != 0 and "overlaps" in err()
    arr = lambda *xs: (p * len(xs))(*[p(x) for x in xs])
    for fn in (lib.bsp_factor_adjoint_up_to_batched_f64, lib.bsp_factor_adjoint_up_to_batched_f32):
        assert fn(h, arr(P.data_ptr()), arr(g.data_ptr()), ctypes.c_int32(0), sp) != 0 and "empty" in err()
        assert fn(h, arr(P.data_ptr(), P.data_ptr()), arr(g.data_ptr(), g.data_ptr() + 8), ctypes.c_int32(2), sp) != 0
        assert "overlap" in err()
    torch.cuda.synchronize()
    assert (g == 0).all() and (P == 1).all()


# ---- dense extraction ----------------------------------------------------------------------------
def _forest_two_roots():
    """two independent blocks (two roots): the trailing pattern behind a cut below both is not full"""
    cols = []
    for base, w in ((0, 12), (12, 9)):
        for c in range(w):
            cols.append(list(range(base + c, base + w)))
    sizes = np.asarray([7, 5, 9, 8, 6, 7, 5, 9, 8, 6, 7, 5] + [6, 7, 5, 9, 8, 6, 7, 5, 9], dtype=np.int64)
    from baspacho_amd import testing as T
    st = B.Settings(findSparseEliminationRanges=False)
    return B.create_solver(st, sizes, T.columns_to_structure(cols), [])


def _dense_cases():
    out = [("forest2", _forest_two_roots())]
    for name in ("mixed_owners", "width129", "forest"):
        out.append((name, build_case(name)[0]))
    out.append(("lump_over_lump", lump_over_lump(300, 70)))
    out.append(("bipartite", bipartite(120, 7, 3, 6, seed=4)))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_schur_to_dense_copies_the_trailing_block(dtype):
    seen_m, seen_zero_tile = set(), False
    for name, sol in _dense_cases():
        data = lbar_random(sol, 9, dtype)  # any values: the kernel only copies
        dev = to_dev(data)
        n = sol.order()
        want_all = sol.densify(data.astype(np.float64), fill_upper_half=True)
        i, j = element_coords(sol)
        for span in [s for s in splits(sol) if s < sol.numSpans()]:
            bar = bar_of(sol, span)
            m = n - bar
            seen_m.add(m)
            want = want_all[bar:, bar:].astype(dtype)
            seen_zero_tile |= m > 64 and bool((want == 0).any())
            rng = np.random.default_rng(m)
            for dest in (None, rng.permutation(m).astype(np.int32)):
                out = torch.full((m, m), float("nan"), dtype=TDT[dtype], device="cuda")
                ret = sol.schurComplement(dev, span, out=out, dest=None if dest is None else to_dev(dest))
                assert ret is out
                got = out.cpu().numpy()
                w = want
                if dest is not None:
                    w = np.empty_like(want)
                    w[np.ix_(dest, dest)] = want
                assert np.array_equal(got, w), (name, span, dest is not None)
            outs = sol.schurComplement([dev, dev.clone()], span)
            assert all(np.array_equal(o.cpu().numpy(), want) for o in outs)
    assert seen_zero_tile


@pytest.mark.parametrize("m", [1, 63, 64, 65, 200])
def test_schur_to_dense_sizes(m):
    """trailing blocks around the 64 x 64 output tile (fp64, internal order; fp32 and dest are covered by
    test_schur_to_dense_copies_the_trailing_block)"""
    sol = lump_over_lump(40, m, below_span=min(7, m))
    hit = [s for s in splits(sol) if sol.order() - bar_of(sol, s) == m]
    assert hit, "no cut with a trailing block of %d" % m
    span = hit[0]
    bar = bar_of(sol, span)
    data = lbar_random(sol, m)
    out = torch.full((m, m), float("nan"), dtype=torch.float64, device="cuda")
    sol.schurComplement(to_dev(data), span, out=out)
    assert np.array_equal(out.cpu().numpy(), sol.densify(data, fill_upper_half=True)[bar:, bar:])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_schur_from_dense_is_the_adjoint(dtype):
    eps = np.finfo(dtype).eps
    for name, sol in _dense_cases():
        n = sol.order()
        i, j = element_coords(sol)
        for span in [s for s in splits(sol) if s < sol.numSpans()][:6]:
            bar = bar_of(sol, span)
            m = n - bar
            rng = np.random.default_rng(span + 1)
            Gd = rng.uniform(-1, 1, (m, m)).astype(dtype)
            for dest in (None, rng.permutation(m).astype(np.int32)):
                Gi = Gd if dest is None else Gd[np.ix_(dest, dest)]  # in internal order
                full = np.zeros((n, n))
                full[bar:, bar:] = Gi.astype(np.float64)
                want = project(sol, full, (i, j))
                out = torch.full((sol.dataSize(),), float("nan"), dtype=TDT[dtype], device="cuda")
                sol.schurComplementAdjoint(to_dev(Gd), span, out=out, dest=None if dest is None else to_dev(dest))
                got = out.cpu().numpy()
                assert np.array_equal(got[i == j], want[i == j].astype(dtype)), (name, span)
                assert (got[(j < bar) | (i < j)] == 0).all(), (name, span)
                assert (np.abs(got - want) <= eps * np.abs(want)).all(), (name, span)
