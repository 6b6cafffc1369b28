"""GPU: blocks of A^-1 on and off the pattern of L by reach solves (Solver.halfInverseColumns /
inverseColumns / inverseBlocks / jointMarginal) against np.linalg.inv of the matrix
as stored (selinv_ref.dense_reference), in correlation units |got - want| / sqrt(want_ii want_jj).

Explicit skeletons put the queries at every place where reachSolveL takes another path: lumps of width 1,
16, 63 and 64 below the cut and 65 at the cut, params of width 1, 16 and 17 (the group split), a query at a
nonzero offset of a lump of several spans, a query in the last lump (whose reach is itself), a query beyond
the cut (no workgroup), roots with no rows below, and two trees of a forest (the block must be exactly 0)."""
import functools

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from buffer_edges import framed, poison_upper
from helpers import solver_random, spd_data, to_dev
from kf_structures import reach_widths
from selinv_ref import SkelBuilder, dense_reference

pytestmark = pytest.mark.gpu

# 10x the worst value of the first MI355X run over this file and test_sparse_cross_covariance_gpu.py
# (fp64 1.33e-15, fp32 7.68e-7, the worst block entry in correlation units); REF_RES bounds max|A X - I| of
# the reference.  Selected inversion's bounds on the same kind of data are 2.5e-14 and 1e-5
TOL = {np.float64: 1.33e-14, np.float32: 7.7e-6}
REF_RES = 1e-14
DTYPES = [np.float64, np.float32]


# ---- structures ----------------------------------------------------------------------------------
_widths = reach_widths  # (kf_structures.py: shared with tests/test_history_gpu.py)


def _forest():
    """three trees without a wide lump: a chain of small lumps, a child below a 64-wide root, a lone lump"""
    b = SkelBuilder()
    chain = [b.lump([2, 1]) for _ in range(5)]
    for a, c in zip(chain, chain[1:]):
        b.couple(a, c)
    child = b.lump([4, 17, 3])
    root = b.lump([16, 40, 8])
    b.couple(child, root)
    b.lump([9, 1])
    return b.solver()


def _random():
    return solver_random(60, fill=0.05, elim=(0, 50), ranges=[0, 50])[0]


def _grid():
    """lumps of width 12, 16, 60, 60, 64 below the cut, 132 and 168 behind it"""
    ss = T.gen_grid(16, 16, 1.0, 2, 37)
    return B.create_solver(B.Settings(), np.full(ss.order(), 2, dtype=np.int64), ss)


def _deep():
    """a sparser grid: two elimination ranges of 2-wide lumps, reaches of several lumps, wide lumps behind"""
    ss = T.gen_grid(20, 20, 1.0, 1, 37)
    return B.create_solver(B.Settings(), np.full(ss.order(), 2, dtype=np.int64), ss)


def _bipartite():
    """points (3) in a given elimination range, cameras (9) in one wide lump right behind it"""
    sizes, ss, _, _ = T.gen_bal_synthetic(num_cams=12, num_pts=80, band=4, seed=3)
    return B.create_solver(B.Settings(), sizes, ss, [0, 80])


STRUCTURES = {"widths": _widths, "forest": _forest, "random": _random, "grid": _grid, "deep": _deep,
              "bipartite": _bipartite}


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """(solver, data, factor on the device, reference inverse in internal order): built once, never changed"""
    import torch
    sol = STRUCTURES[name]()
    data = spd_data(sol, 17, dtype=dtype)
    _, X, res = dense_reference(sol, data)
    assert res < REF_RES, res
    L = to_dev(data)
    sol.factor(L)
    torch.cuda.synchronize()
    return sol, data, L, X


def _scalars(sol, prm):
    ss = sol.skel()["spanStart"]
    s = int(sol.paramToSpan()[prm])
    return np.arange(int(ss[s]), int(ss[s + 1]))


def _lump_of(sol, prm):
    return int(sol.skel()["spanToLump"][int(sol.paramToSpan()[prm])])


def _block_error(sol, X, pairs, blocks):
    d = np.diag(X)
    worst = 0.0
    for (p, q), blk in zip(pairs, blocks):
        r, c = _scalars(sol, p), _scalars(sol, q)
        got = blk.cpu().numpy().astype(np.float64)
        assert got.shape == (len(r), len(c))
        assert np.isfinite(got).all(), (p, q)
        worst = max(worst, float((np.abs(got - X[np.ix_(r, c)]) / np.sqrt(np.outer(d[r], d[c]))).max()))
    return worst


def _report(tag, dtype, err):
    print("invblk-err %s %s %.3e" % (tag, np.dtype(dtype).name, err))
    assert err < TOL[dtype], (tag, err)


def _all_pairs(params):
    return [(p, q) for p in params for q in params]


def _off_pattern(sol, pairs):
    """pairs of params that share no stored block"""
    out = []
    for p, q in pairs:
        try:
            sol.blockOffset(p, q)
        except RuntimeError:
            out.append((p, q))
    return out


# ---- kernel shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_widths_every_pair(dtype):
    """every pair of params of the `widths` skeleton: query lumps 1, 16, 63, 64 wide, the cut at the 65
    wide one, queries behind it, params 1, 16 and 17 wide, nonzero offsets inside a lump"""
    sol, _, L, X = _case("widths", dtype)
    plan = sol._testReachPlan(list(range(sol.numSpans())))
    widths = np.diff(sol.skel()["lumpStart"]).tolist()
    assert widths == [1, 16, 63, 64, 65, 7] and plan["cutLump"] == 4
    assert sorted({g["k"] for g in plan["groups"]}) == [1, 5, 7, 8, 16]  # 17 = 16 + 1, 24 = 16 + 8, 40 = 16 + 16 + 8
    assert len(plan["units"]) == 65 + 7  # the queries at and behind the cut have no workgroup
    assert any(g["row0"] > sol.skel()["lumpStart"][g["firstLump"]] for g in plan["groups"])
    pairs = _all_pairs(range(sol.numSpans()))
    _report("widths", dtype, _block_error(sol, X, pairs, sol.inverseBlocks(L, pairs)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_forest_zero_blocks_and_roots(dtype):
    import torch
    sol, _, L, X = _case("forest", dtype)
    n = sol.numSpans()
    plan = sol._testReachPlan(list(range(n)))
    assert plan["cutLump"] == sol.numLumps() and not plan["units"]
    last = plan["queries"][n - 1]
    assert last["reach"].tolist() == [sol.numLumps() - 1]  # the last lump: its reach is itself
    pairs = _all_pairs(range(n))
    blocks = sol.inverseBlocks(L, pairs)
    _report("forest", dtype, _block_error(sol, X, pairs, blocks))
    # params of different trees: exactly 0, not merely small
    tree = np.repeat([0, 1, 2], [5, 2, 1])
    crossed = 0
    for (p, q), blk in zip(pairs, blocks):
        if tree[_lump_of(sol, p)] != tree[_lump_of(sol, q)]:
            assert not bool(torch.count_nonzero(blk)), (p, q)
            crossed += 1
    assert crossed > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["random", "grid", "deep", "bipartite"])
def test_structures(name, dtype):
    """random pairs on a random structure with an elimination range, a grid with wide trailing lumps, a
    sparser grid with reaches of several lumps through two elimination ranges, and a bipartite points /
    cameras problem with a given elimination range (point-point, point-camera and camera-camera pairs)"""
    sol, _, L, X = _case(name, dtype)
    rng = np.random.default_rng(5)
    n = sol.numSpans()
    prm = rng.choice(n, size=min(n, 24), replace=False).tolist()
    if name == "bipartite":
        prm = prm[:16] + [80, 85, 91]  # cameras: beyond the cut, which sits right behind the range
        plan = sol._testReachPlan(prm)
        assert plan["cutLump"] == 80 and sol.sparseEliminationRanges().tolist() == [0, 80]
        assert plan["groups"] and plan["units"]
    if name == "deep":
        plan = sol._testReachPlan(prm)
        assert len(sol.sparseEliminationRanges()) == 3 and max(len(q["reach"]) for q in plan["queries"]) >= 3
    pairs = _all_pairs(prm)
    assert len(_off_pattern(sol, pairs)) > len(pairs) // 4
    _report(name, dtype, _block_error(sol, X, pairs, sol.inverseBlocks(L, pairs)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_and_full_columns(dtype):
    """W = L^-1 E against numpy, exactly 0 outside the reach of each column; inverseColumns against inv(A)"""
    sol, data, L, X = _case("widths", dtype)
    A = sol.densify(np.asarray(data).astype(np.float64), fill_upper_half=True)
    Lc = np.linalg.cholesky(A)
    prm = [0, 3, 1, 9, 2, 12, 0]  # stacked in the order given, a repeat included
    idx = np.concatenate([_scalars(sol, p) for p in prm])
    want = np.linalg.solve(Lc, np.eye(sol.order())[:, idx]).T
    W = sol.halfInverseColumns(L, prm).cpu().numpy().astype(np.float64)
    assert W.shape == want.shape
    d = np.diag(X)
    # |w_c|^2 = X_cc: sqrt(X_cc) is the scale of the entries of column c
    _report("half", dtype, float((np.abs(W - want) / np.sqrt(d[idx])[:, None]).max()))
    # rows outside the reach: exactly 0
    plan = sol._testReachPlan(prm)
    ls = sol.skel()["lumpStart"]
    col = 0
    for q in plan["queries"]:
        inside = np.zeros(sol.order(), dtype=bool)
        for l in q["reach"]:
            inside[int(ls[l]):int(ls[l + 1])] = True
        inside[int(ls[plan["cutLump"]]):] = True
        assert not W[col:col + q["width"], ~inside].any(), q
        col += q["width"]
    Xc = sol.inverseColumns(L, prm).cpu().numpy().astype(np.float64)
    _report("columns", dtype, float((np.abs(Xc - X[idx, :]) / np.sqrt(np.outer(d[idx], d))).max()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_pattern_pairs_agree_with_selected_inverse(dtype):
    """P == Q against marginals(), on-pattern pairs against the blocks of selectedInverse: the two routes
    agree within the same TOL that bounds each against the reference (first MI355X run: fp64 5.5e-16,
    fp32 3.0e-7)"""
    import torch
    sol, _, L, X = _case("random", dtype)
    Z = L.clone()
    sol.selectedInverse(Z)
    n = sol.numSpans()
    prm = list(range(0, n, 3))
    diag = sol.inverseBlocks(L, [(p, p) for p in prm])
    marg = sol.marginals(Z, prm)
    d = np.diag(X)
    worst = 0.0
    for p, a, m in zip(prm, diag, marg):
        sc = np.sqrt(np.outer(d[_scalars(sol, p)], d[_scalars(sol, p)]))
        worst = max(worst, float((np.abs((a - m).cpu().numpy().astype(np.float64)) / sc).max()))
    on = [(p, q) for p in range(n) for q in range(p) if not _off_pattern(sol, [(p, q)])][:40]
    assert len(on) >= 10
    blocks = sol.inverseBlocks(L, on)
    Zh = Z.cpu().numpy().astype(np.float64)
    for (p, q), blk in zip(on, blocks):
        o, st, fl = sol.blockOffset(p, q)
        r, c = _scalars(sol, p), _scalars(sol, q)
        if fl:
            z = np.array([[Zh[o + j * st + i] for j in range(len(c))] for i in range(len(r))])
        else:
            z = np.array([[Zh[o + i * st + j] for j in range(len(c))] for i in range(len(r))])
        sc = np.sqrt(np.outer(d[r], d[c]))
        worst = max(worst, float((np.abs(blk.cpu().numpy().astype(np.float64) - z) / sc).max()))
    print("invblk-err vs-selinv %s %.3e" % (np.dtype(dtype).name, worst))
    assert worst < TOL[dtype], worst
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_joint_marginal(dtype):
    import torch
    sol, _, L, X = _case("grid", dtype)
    prm = [3, 200, 17, 120, 255, 64]
    C = sol.jointMarginal(L, prm)
    idx = np.concatenate([_scalars(sol, p) for p in prm])
    assert C.shape == (len(idx), len(idx))
    assert torch.equal(C, C.t())  # symmetric to the last bit
    torch.linalg.cholesky(C)      # raises if C is not positive definite
    d = np.diag(X)
    got = C.cpu().numpy().astype(np.float64)
    _report("joint", dtype, float((np.abs(got - X[np.ix_(idx, idx)]) / np.sqrt(np.outer(d[idx], d[idx]))).max()))


def test_chunks_of_512_columns():
    """more distinct columns than one call takes: the chunked result is bitwise the pair-by-pair result"""
    import torch
    sol, _, L, X = _case("deep", np.float64)
    assert sol.INVERSE_BLOCKS_MAX_COLUMNS == 512
    rng = np.random.default_rng(2)
    pairs = [(int(a), int(b)) for a, b in rng.choice(sol.numSpans(), size=(400, 2))]
    assert 2 * len({p for pq in pairs for p in pq}) > 512
    blocks = sol.inverseBlocks(L, pairs)
    assert blocks.shape == (400, 2, 2)
    _report("chunks", np.float64, _block_error(sol, X, pairs, blocks))
    for k in (0, 150, 399):
        assert torch.equal(blocks[k], sol.inverseBlocks(L, [pairs[k]])[0])


# ---- contract ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_framed_poisoned_buffers_other_stream_reproducible(dtype):
    """L, out and W inside sentinel frames at odd offsets, the strictly-upper elements of L poisoned, on a
    non-default stream: nothing outside out / W is written, L is bitwise unchanged, the results are bitwise
    the plain call's, and two runs agree bitwise"""
    import torch
    sol, data, L, X = _case("widths", dtype)
    pairs = _all_pairs([0, 2, 3, 9, 12, 13])
    prm = [2, 9, 12, 0]
    plain = sol.inverseBlocks(L, pairs)
    plain_w = sol.halfInverseColumns(L, prm)
    torch.cuda.synchronize()
    n_out = sum(b.numel() for b in plain)
    n_w = plain_w.numel()
    lh = poison_upper(L.cpu().numpy().copy(), sol)
    fr = framed(dtype, [lh, np.zeros(n_out, dtype=dtype), np.zeros(n_w, dtype=dtype)])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    sol.setStream(stream)
    try:
        with torch.cuda.stream(stream):
            runs = []
            for _ in range(2):
                got = sol.inverseBlocks(fr.view(0), pairs, out=fr.view(1))
                w = sol.halfInverseColumns(fr.view(0), prm, out=fr.view(2))
                runs.append((torch.cat([g.reshape(-1) for g in got]).clone(), w.clone()))
        stream.synchronize()
    finally:
        sol.setStream(None)
    fr.assert_intact(read_only=[0], what="inverseBlocks / halfInverseColumns")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0], torch.cat([b.reshape(-1) for b in plain]))
    assert torch.equal(runs[0][1], plain_w)
    _report("framed", dtype, _block_error(sol, X, pairs, sol.inverseBlocks(L, pairs)))


def test_arguments_are_checked():
    import torch
    sol, _, L, _ = _case("forest", np.float64)
    with pytest.raises(IndexError):
        sol.inverseBlocks(L, [(0, sol.numSpans())])
    with pytest.raises(IndexError):
        sol.halfInverseColumns(L, [-1])
    with pytest.raises(ValueError):
        sol.inverseBlocks(L[:-1], [(0, 0)])
    with pytest.raises(ValueError):
        sol.inverseBlocks(L, [(0, 0)], out=torch.empty(3, dtype=L.dtype, device=L.device))
    assert sol.inverseBlocks(L, []) == []
    assert sol.halfInverseColumns(L, []).shape == (0, sol.order())
    # the C entry refuses what the Python layer cannot produce
    import ctypes
    bad = np.array([0, 2], dtype=np.int64)  # block 0 is 3 x 3 = 9 elements
    zero = np.zeros(1, dtype=np.int64)
    out = torch.empty(16, dtype=L.dtype, device=L.device)
    i64p = ctypes.POINTER(ctypes.c_int64)
    rc = sol._lib.bsp_inverse_blocks_f64(sol._h, ctypes.c_void_p(L.data_ptr()), ctypes.c_int64(1),
                                         zero.ctypes.data_as(i64p), zero.ctypes.data_as(i64p),
                                         ctypes.c_void_p(out.data_ptr()), bad.ctypes.data_as(i64p))
    assert rc != 0 and b"output offsets" in sol._lib.bsp_last_error()
    rc = sol._lib.bsp_reach_solve_l_f64(sol._h, None, ctypes.c_int64(1), zero.ctypes.data_as(i64p),
                                        ctypes.c_void_p(out.data_ptr()))
    assert rc != 0 and b"NULL" in sol._lib.bsp_last_error()
    part = solver_random(60, fill=0.05, elim=(0, 50), ranges=[0, 50], policy=B.AddFillForGivenElims)[0]
    assert part.canFactorUpToSpan() < part.numSpans()
    with pytest.raises(RuntimeError, match="can only factor up to span"):
        part.inverseBlocks(torch.zeros(part.dataSize(), dtype=torch.float64, device="cuda"), [(0, 0)])
