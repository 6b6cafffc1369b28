"""CPU: the math, the storage and the plan of the partial factor's reverse mode
before any GPU run.  The numpy restatement (partial_adjoint_ref.recurrence_np: seed, the node
recurrence over the re-levelled plan of the cut, final pass) matches dense torch autograd of
[L11 0; L21 tril(S)] on every selinv_cases.py skeleton and on random structures with elimination
ranges, at every admissible split; the plan of a cut has the properties the sweep relies on."""
import numpy as np
import pytest

from autograd_ref import element_coords
from chol_adjoint_ref import lbar_random, rel_error
from helpers import solver_random
from kf_structures import bipartite
from known_factor import known_factor_data
from partial_adjoint_ref import oracle, plan_records, recurrence_np, splits
from selinv_cases import build_case, case_names

TOL = 1e-11  # test_chol_adjoint_ref_cpu.py's bound: fp64 recurrence against the fp64 oracle


def _check_all_splits(sol, seed):
    data = known_factor_data(sol, seed, np.float64, rho=0.5).data
    coords = element_coords(sol)
    i, j = coords
    for span in splits(sol):
        pbar = lbar_random(sol, seed + 17 + span)
        want, P = oracle(sol, data, pbar, span, coords)
        got = recurrence_np(sol, P, pbar, span)
        err = rel_error(got, want)
        print("span %d / %d: %.2e" % (span, sol.numSpans(), err))
        assert err < TOL, (span, err)
        assert (got[i < j] == 0).all()
        if span == 0:
            assert np.array_equal(got, np.where(i >= j, pbar, 0.0))


def _check_plan(sol, span):
    sk = sol.skel()
    cut = int(sk["spanToLump"][span]) if span < sol.numSpans() else sol.numLumps()
    full, part = sol._testSelInvPlan(), sol._testSelInvPlan(span)
    lf, lp = plan_records(full), plan_records(part)
    assert set(lp) == {k for k in lf if k[0] < cut}, span
    assert part["numLevels"] == (max(lp.values()) + 1 if lp else 0)
    done = {}
    for (lump, c0, w, r, nRest), lev in lp.items():
        done[lump] = max(done.get(lump, -1), lev)
    cp, crs, s2l = sk["chainColPtr"], sk["chainRowSpan"], sk["spanToLump"]
    for (lump, c0, w, r, nRest), lev in lp.items():
        owners = {int(s2l[crs[c]]) for c in range(int(cp[lump]), int(cp[lump + 1]))} - {lump}
        for J in owners:
            if J < cut:
                assert lev > done[J], (span, lump, J)
        # nodes of one lump right to left, one level each
        if nRest > 0:
            right = [v for k, v in lp.items() if k[0] == lump and k[1] == c0 + w]
            assert right and lev == right[0] + 1
    if lp and cut < sol.numLumps():
        # something starts at once: the levels are counted among the leading lumps alone
        assert min(lp.values()) == 0


@pytest.mark.parametrize("name", case_names())
def test_recurrence_matches_oracle_on_selinv_cases(name):
    sol, _ = build_case(name)
    _check_all_splits(sol, 5)


@pytest.mark.parametrize("seed", [3, 8])
def test_recurrence_matches_oracle_on_random_structures(seed):
    sol, _, _ = solver_random(seed, fill=0.037, elim=(0, 60))
    assert len(sol.sparseEliminationRanges()) >= 2
    _check_all_splits(sol, seed)


@pytest.mark.parametrize("name", case_names())
def test_plan_of_every_cut_on_selinv_cases(name):
    sol, _ = build_case(name)
    for span in splits(sol):
        _check_plan(sol, span)


@pytest.mark.parametrize("seed", [3, 8])
def test_plan_of_every_cut_on_random_structures(seed):
    sol, _, _ = solver_random(seed, fill=0.037, elim=(0, 60))
    for span in splits(sol):
        _check_plan(sol, span)


def test_plan_up_to_the_end_is_the_complete_plan():
    for name in ("mixed_owners", "forest", "width129"):
        sol, _ = build_case(name)
        a, b = sol._testSelInvPlan(), sol._testSelInvPlan(sol.numSpans())
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], dict):
                for f in a[k]:
                    assert np.array_equal(a[k][f], b[k][f]), (name, k, f)
            else:
                assert a[k] == b[k], (name, k)


def test_bipartite_cut_after_the_points_is_one_level_of_small_lumps():
    sol = bipartite(300, 13, 3, 6, seed=5)
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    span = int(sol.skel()["lumpToSpan"][ranges[-1]])
    plan = sol._testSelInvPlan(span)
    assert plan["numLevels"] == 1 and len(plan["node"]["lump"]) == 0
    assert len(plan["small"]["lump"]) == ranges[-1]
    assert sol._testSelInvPlan()["numLevels"] > 1


def test_plan_hook_refuses_what_factor_up_to_refuses():
    sol = bipartite(300, 13, 3, 6, seed=5, ranges=[0, 100, 200, 300])
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    inside = int(sol.skel()["lumpToSpan"][(ranges[0] + ranges[1]) // 2])
    with pytest.raises(RuntimeError, match="sparse-elimination range"):
        sol._testSelInvPlan(inside)
    with pytest.raises(RuntimeError):
        sol._testSelInvPlan(sol.numSpans() + 1)
    wide, _ = build_case("width129")
    off = [s for s in range(wide.numSpans()) if int(wide.skel()["spanOffsetInLump"][s]) != 0]
    if off:
        with pytest.raises(RuntimeError, match="inside a lump"):
            wide._testSelInvPlan(off[0])


def test_entry_points_exist():
    import baspacho_amd as B
    from baspacho_amd import _lib, autograd
    lib = _lib.load()
    for base in ("bsp_factor_adjoint_up_to", "bsp_factor_adjoint_up_to_batched", "bsp_schur_to_dense",
                 "bsp_schur_to_dense_batched", "bsp_schur_from_dense", "bsp_schur_from_dense_batched"):
        for sfx in ("f64", "f32"):
            assert hasattr(lib, "%s_%s" % (base, sfx))
    assert hasattr(lib, "bsp_test_selinv_plan_up_to")
    for name in ("factorAdjointUpTo", "schurComplement", "schurComplementAdjoint"):
        assert callable(getattr(B.Solver, name))
    for name in ("factor_up_to", "schur_complement", "solve_l_up_to"):
        assert callable(getattr(autograd, name)) and name in autograd.__all__
