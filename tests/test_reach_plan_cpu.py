"""CPU: the reach plan (buildReachPlan, read through Solver._testReachPlan(): the plan reachSolveL and
inverseBlocks run, built on the host).  Every reach list against a brute-force closure computed from
skel(), the cut rule, the Gram row ranges against the intersection of the reaches, and the column groups."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from helpers import solver_random
from selinv_cases import build_case, case_names
from selinv_ref import SkelBuilder, split_sizes

WIDE, COLS = 64, 16


def brute_cut(sol):
    sk = sol.skel()
    widths = np.diff(sk["lumpStart"])
    wide = np.nonzero(widths > WIDE)[0]
    cut = int(wide[0]) if len(wide) else sol.numLumps()
    er = sol.sparseEliminationRanges()
    for b, e in zip(er[:-1], er[1:]):
        if b < cut < e:
            cut = int(b)
    return cut


def brute_reach(sol, lump, cut):
    """the closure by repeated sweeps over a boolean mask (no queue, no order assumed)"""
    sk = sol.skel()
    cp, crs, s2l = sk["chainColPtr"], sk["chainRowSpan"], sk["spanToLump"]
    inside = np.zeros(sol.numLumps(), dtype=bool)
    inside[lump] = True
    while True:
        before = int(inside.sum())
        for l in np.nonzero(inside)[0]:
            inside[s2l[crs[int(cp[l]):int(cp[l + 1])]]] = True
        if int(inside.sum()) == before:
            break
    out = np.nonzero(inside)[0]
    return out[out < cut] if lump < cut else out[:0]


def check_plan(sol, params):
    sk = sol.skel()
    ls, ss, s2l = sk["lumpStart"], sk["spanStart"], sk["spanToLump"]
    p2s = sol.paramToSpan()
    plan = sol._testReachPlan(params)
    cut = brute_cut(sol)
    assert plan["cutLump"] == cut
    assert plan["cutSpan"] == int(sk["lumpToSpan"][cut])
    assert (np.diff(ls)[:cut] <= WIDE).all()
    # queries: spans, stacked columns, reach lists
    col, reach = 0, []
    assert len(plan["queries"]) == len(params)
    for prm, q in zip(params, plan["queries"]):
        span = int(p2s[prm])
        assert (q["span"], q["lump"], q["col0"]) == (span, int(s2l[span]), col)
        assert q["width"] == int(ss[span + 1] - ss[span])
        want = brute_reach(sol, q["lump"], cut)
        assert np.array_equal(q["reach"], want), (prm, q["reach"], want)
        reach.append(set(want.tolist()))
        col += q["width"]
    assert plan["numCols"] == col
    # groups: ceil(width / 16) per query below the cut, none at or beyond it; units for the others
    gi, units = 0, []
    for qi, q in enumerate(plan["queries"]):
        if q["lump"] >= cut:
            units += [(q["col0"] + c, int(ss[q["span"]]) + c) for c in range(q["width"])]
            continue
        for c0 in range(0, q["width"], COLS):
            g = plan["groups"][gi]
            gi += 1
            assert (g["query"], g["col0"], g["k"]) == (qi, q["col0"] + c0, min(COLS, q["width"] - c0))
            assert g["row0"] == int(ss[q["span"]]) + c0
            assert g["len"] == len(q["reach"]) and g["firstLump"] == q["lump"]
    assert gi == len(plan["groups"])
    assert plan["units"] == units
    # Gram items: every pair i >= j, rows = the lumps of the intersection below the cut + [cut, order)
    it = iter(plan["items"])
    off = 0
    for i in range(len(params)):
        for j in range(i + 1):
            item = next(it)
            qi, qj = plan["queries"][i], plan["queries"][j]
            assert (item["i"], item["j"]) == (i, j)
            assert (item["colP"], item["nP"], item["colQ"], item["nQ"]) == (qi["col0"], qi["width"], qj["col0"],
                                                                         qj["width"])
            assert item["outOff"] == off
            off += qi["width"] * qj["width"]
            rows = np.zeros(sol.order(), dtype=bool)
            for l in reach[i] & reach[j]:
                rows[int(ls[l]):int(ls[l + 1])] = True
            rows[int(ls[cut]):] = True
            got = np.zeros(sol.order(), dtype=bool)
            last = -1
            for a, b in item["ranges"]:
                assert last < a < b <= sol.order(), item["ranges"]  # ascending, not even adjacent
                assert not got[a:b].any()
                got[a:b] = True
                last = b
            assert np.array_equal(got, rows), (i, j)
            assert item["rows"] == int(rows.sum())
    return plan


def _some_params(sol, seed, count=12):
    rng = np.random.default_rng(seed)
    n = sol.numSpans()
    prm = rng.choice(n, size=min(count, n), replace=False).tolist()
    # the first and the last span of the internal order, whichever params they are, and a repeat
    p2s = sol.paramToSpan()
    inv = np.argsort(p2s)
    return prm + [int(inv[0]), int(inv[-1]), prm[0]]


@pytest.mark.parametrize("seed", [60, 61, 62])
def test_random_structures(seed):
    sol, _, _ = solver_random(seed, fill=0.05, elim=(0, 50), ranges=[0, 50])
    plan = check_plan(sol, _some_params(sol, seed))
    assert any(len(q["reach"]) > 1 for q in plan["queries"])


@pytest.mark.parametrize("name", case_names())
def test_selinv_skeletons(name):
    sol, _ = build_case(name)
    check_plan(sol, _some_params(sol, 3, count=6))


def test_grid():
    ss = T.gen_grid(12, 12, 1.0, 2, 37)
    sol = B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)
    plan = check_plan(sol, _some_params(sol, 5, count=20))
    # with 3-wide params the supernodes of this grid are all wider than 64: the cut is lump 0
    assert plan["cutLump"] == 0 and not plan["groups"] and len(plan["units"]) == plan["numCols"]
    # a sparser grid: two elimination ranges of narrow lumps, reaches of several lumps, wide lumps behind
    ss = T.gen_grid(20, 20, 1.0, 1, 37)
    sol = B.create_solver(B.Settings(), np.full(ss.order(), 2, dtype=np.int64), ss)
    assert len(sol.sparseEliminationRanges()) == 3 and 0 < brute_cut(sol) < sol.numLumps()
    plan = check_plan(sol, _some_params(sol, 5, count=20))
    assert max(len(q["reach"]) for q in plan["queries"]) >= 3


def test_forest_is_disjoint():
    """block-diagonal: the reaches of two trees do not meet, no lump is wide: no rows at all"""
    b = SkelBuilder()
    trees = []
    for _ in range(3):
        chain = [b.lump([2, 3]) for _ in range(4)]
        for a, c in zip(chain, chain[1:]):
            b.couple(a, c)
        trees.append(chain)
    sol = b.solver()
    sk = sol.skel()
    first = [int(sk["lumpToSpan"][t[0]]) for t in trees]
    plan = check_plan(sol, first)
    assert plan["cutLump"] == sol.numLumps()
    for item in plan["items"]:
        assert (item["rows"] == 0) == (item["i"] != item["j"]), item


def _elim_solver(width_elim, n_elim, tail_sizes):
    """n_elim independent lumps of `width_elim` (one elimination range), all coupled to the lumps of
    tail_sizes behind them"""
    b = SkelBuilder()
    heads = [b.lump(split_sizes(width_elim, [5, 7])) for _ in range(n_elim)]
    tails = [b.lump(split_sizes(w, [9, 4])) for w in tail_sizes]
    for h in heads:
        b.couple(h, *tails)
    for a, c in zip(tails, tails[1:]):
        b.couple(a, c)
    span_start = np.concatenate([[0], np.cumsum(b.sizes)]).astype(np.int64)
    ref = b.solver()
    sk = ref.skel()
    # the same skeleton with the heads as one sparse-elimination range
    col_ptr, row_ind = [0], []
    for l in range(ref.numLumps()):
        row_ind += sk["chainRowSpan"][int(sk["chainColPtr"][l]):int(sk["chainColPtr"][l + 1])].tolist()
        col_ptr.append(len(row_ind))
    return B.Solver.from_skeleton(span_start, b.l2s, col_ptr, row_ind, [0, n_elim]), heads, tails


def test_cut_right_behind_an_elimination_range():
    sol, heads, tails = _elim_solver(23, 6, [65, 30])
    assert sol.sparseEliminationRanges().tolist() == [0, 6]
    plan = check_plan(sol, list(range(sol.numSpans()))[::3])
    assert plan["cutLump"] == tails[0] == 6  # the wide lump itself: a range ends where the cut begins


def test_cut_lowered_to_the_beginning_of_a_range():
    """the elimination lumps themselves are 23 wide, one of them 70: the cut is the range's first lump"""
    b = SkelBuilder()
    pre = [b.lump([4]) for _ in range(2)]
    heads = [b.lump(split_sizes(70 if i == 3 else 23, [5, 7])) for i in range(6)]
    tail = b.lump([20, 12])
    for h in pre + heads:
        b.couple(h, tail)
    ref = b.solver()
    sk = ref.skel()
    col_ptr, row_ind = [0], []
    for l in range(ref.numLumps()):
        row_ind += sk["chainRowSpan"][int(sk["chainColPtr"][l]):int(sk["chainColPtr"][l + 1])].tolist()
        col_ptr.append(len(row_ind))
    span_start = np.concatenate([[0], np.cumsum(b.sizes)]).astype(np.int64)
    sol = B.Solver.from_skeleton(span_start, b.l2s, col_ptr, row_ind, [2, 8])
    plan = check_plan(sol, list(range(sol.numSpans()))[::2])
    assert plan["cutLump"] == 2 and int(np.diff(sk["lumpStart"])[5]) == 70
    assert any(q["lump"] < 2 for q in plan["queries"]) and any(2 <= q["lump"] < 5 for q in plan["queries"])


def test_elimination_lumps_23_wide_stay_below_the_cut():
    sol, heads, tails = _elim_solver(23, 6, [40, 30])
    plan = check_plan(sol, list(range(sol.numSpans()))[::3])
    assert plan["cutLump"] == sol.numLumps()
    assert not plan["units"]


def test_groups_split_at_16_columns():
    b = SkelBuilder()
    h = b.lump([1, 16, 17])
    t = b.lump([33, 5])
    b.couple(h, t)
    sol = b.solver()
    plan = check_plan(sol, [0, 1, 2, 3, 4])
    assert [g["k"] for g in plan["groups"]] == [1, 16, 16, 1, 16, 16, 1, 5]
    assert [g["row0"] for g in plan["groups"]] == [0, 1, 17, 33, 34, 50, 66, 67]


def test_arguments_are_checked():
    sol, _, _ = solver_random(60, fill=0.05)
    with pytest.raises(RuntimeError, match="not in"):
        sol._testReachPlan([sol.numSpans()])
    part, _, _ = solver_random(60, fill=0.05, elim=(0, 50), ranges=[0, 50], policy=B.AddFillForGivenElims)
    assert part.canFactorUpToSpan() < part.numSpans()
    with pytest.raises(RuntimeError, match="can only factor up to span"):
        part._testReachPlan([0])
