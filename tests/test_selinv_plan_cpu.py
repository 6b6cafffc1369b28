"""CPU: invariants of the selected-inversion plan (buildSelInvPlan, read through
Solver._testSelInvPlan(): the plan selectedInverse() runs, built on the host).  Coverage of every lump,
the small-path predicate evaluated independently from skel(), level order against the lumps owning a
lump's chain rows, the split-K chunks of the Z_RR U product, and the scratch sizes."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from helpers import solver_random
from selinv_cases import NODE_W, SMALL_CHAINS, SMALL_ELEMS, SMALL_W, build_case, case_names


def _lump_shape(sk, l):
    """(width, chains below the diagonal block, rows below it) from the skeleton"""
    ls, ss, cp, crs, s2l = sk["lumpStart"], sk["spanStart"], sk["chainColPtr"], sk["chainRowSpan"], \
        sk["spanToLump"]
    below = [int(s) for s in crs[int(cp[l]):int(cp[l + 1])] if s2l[s] != l]
    return int(ls[l + 1] - ls[l]), below, int(sum(ss[s + 1] - ss[s] for s in below))


def check_plan(sol):
    sk = sol.skel()
    p = sol._testSelInvPlan()
    sm, nd = p["small"], p["node"]
    nl = sol.numLumps()
    s2l = sk["spanToLump"]
    # launch order: levels never decrease
    assert (np.diff(sm["level"]) >= 0).all() and (np.diff(nd["level"]) >= 0).all()
    first, last = np.full(nl, -1), np.full(nl, -1)
    for l in range(nl):
        width, below, r = _lump_shape(sk, l)
        k = len(below)
        small = width <= SMALL_W and k <= SMALL_CHAINS and r * width <= SMALL_ELEMS
        si = np.nonzero(sm["lump"] == l)[0]
        ni = np.nonzero(nd["lump"] == l)[0]
        if small:
            # eligibility (both directions) and the item's own shape
            assert len(si) == 1 and len(ni) == 0, (l, width, k, r)
            i = si[0]
            assert (sm["n"][i], sm["k"][i], sm["r"][i]) == (width, k, r), l
            first[l] = last[l] = sm["level"][i]
            continue
        assert len(si) == 0 and len(ni) > 0, (l, width, k, r)
        # coverage: nodes right to left on consecutive levels, [0, width) without gaps or overlaps,
        # only the rightmost may be narrower than NODE_W
        c0, w, lev = nd["c0"][ni], nd["w"][ni], nd["level"][ni]
        assert c0[-1] == 0 and c0[0] + w[0] == width, (l, c0, w)
        assert (c0[:-1] == c0[1:] + w[1:]).all(), (l, c0, w)
        assert (w[1:] == NODE_W).all() and 0 < w[0] <= NODE_W, (l, w)
        assert (np.diff(lev) == 1).all(), (l, lev)
        assert (nd["nRest"][ni] == width - c0 - w).all()
        assert (nd["r"][ni] == nd["nRest"][ni] + r).all()
        first[l], last[l] = lev[0], lev[-1]
    # dependencies: a lump starts after every lump that owns one of its chain-row spans is done
    for l in range(nl):
        for s in _lump_shape(sk, l)[1]:
            J = int(s2l[s])
            assert J > l and first[l] > last[J], (l, J, first[l], last[J])
    # split-K and tiles
    r, kc, nk, nt = nd["r"], nd["kChunk"], nd["nk"], nd["nTiles"]
    assert (kc % 16 == 0).all()
    pos = r > 0
    assert (nk[pos] * kc[pos] >= r[pos]).all() and (r[pos] > (nk[pos] - 1) * kc[pos]).all()
    assert (nk[~pos] == 0).all()
    assert (nt == (r + 63) // 64).all()
    # a node with r = 0 is the rightmost block of a lump with nothing below: a root, level 0
    assert (nd["level"][~pos] == 0).all()
    # scratch: each level's U, partial products, per-tile U^T Z and per-node Linv fit what is allocated
    for L in range(p["numLevels"]):
        at = nd["level"] == L
        assert int((r[at] * NODE_W).sum()) <= p["uElems"], L
        assert int((nk[at] * r[at] * NODE_W).sum()) <= p["pElems"], L
        assert int((nt[at] * NODE_W * NODE_W).sum()) <= p["wElems"], L
        assert int(at.sum()) * NODE_W * NODE_W <= p["linvElems"], L
        # tiles of a level are numbered consecutively, node by node
        tb = nd["tileBase"][at]
        assert (tb == np.concatenate([[0], np.cumsum(nt[at])[:-1]])).all(), L
    levels = set(sm["level"].tolist()) | set(nd["level"].tolist())
    assert levels == set(range(p["numLevels"]))
    return p


@pytest.mark.parametrize("name", case_names())
def test_explicit_skeletons(name):
    sol, expect = build_case(name)
    expect(check_plan(sol))


@pytest.mark.parametrize("seed", range(57, 63))
def test_random_structures(seed):
    check_plan(solver_random(seed, find_ranges=bool(seed % 2))[0])
    check_plan(solver_random(seed, fill=0.03, elim=(0, 60), ranges=[0, 60])[0])


def test_grid_and_meridians():
    ss = T.gen_grid(40, 40, 1.0, 2, 37)
    check_plan(B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss))
    ss = T.gen_meridians(4, 150, 0.5, 12, 60, 2, 2, 37)
    check_plan(B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss))


def test_plan_is_the_one_of_the_skeleton():
    """the view needs no device and is deterministic; a solver rebuilt from its serialized plan has
    the same selected-inversion plan"""
    sol, _, _ = solver_random(58, fill=0.05, elim=(0, 40))
    a, b = sol._testSelInvPlan(), sol._testSelInvPlan()
    c = B.Solver.from_plan(sol.serialize_plan())._testSelInvPlan()
    for x in (b, c):
        for part in ("small", "node"):
            for f in a[part]:
                assert np.array_equal(a[part][f], x[part][f]), (part, f)
