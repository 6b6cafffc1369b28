"""GPU: selected inversion (Solver.selectedInverse / bsp_selected_inverse_*): Z = A^-1 on the block
pattern of L, written over the factor.  Small problems against np.linalg.inv of the dense matrix (every
stored entry, the upper triangles of the diagonal blocks included: they are written full); BAL-871 at
full size against the library's own solve() with identity right-hand sides."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from helpers import solver_random, spd_data, to_dev
from selinv_ref import corr_error, dense_reference
from oracle import cref

pytestmark = pytest.mark.gpu

# worst error over every stored entry in correlation units, |got - want| / sqrt(want_ii want_jj)
# (selinv_ref.py): never weaker than the max-normalised error at the same number
# 10x the worst value of the first MI355X runs (fp64 2.6e-15, fp32 1.2e-6, worst entry over
# test_selinv_gpu.py and test_selinv_edges_gpu.py); REF_RES bounds max|A X - I| of the reference
TOL = {np.float64: 2.5e-14, np.float32: 1e-5}
REF_RES = 1e-14


def _selinv(sol, data):
    import torch
    d = to_dev(data)
    sol.factor(d)
    sol.selectedInverse(d)
    torch.cuda.synchronize()
    return d


def _check_dense(sol, dtype, seed=5, beta_factor=1.5):
    data = spd_data(sol, seed, beta_factor=beta_factor, dtype=dtype)
    _, want, res = dense_reference(sol, data)     # inv() of the input as stored (fp32: rounded)
    assert res < REF_RES, res
    got = _selinv(sol, data).cpu().numpy().astype(np.float64)
    err = corr_error(sol, got, want)
    print("selinv-err %s %s" % (np.dtype(dtype).name, err))
    assert err.value < TOL[dtype], err
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_structures(dtype):
    for i in range(4):
        sol, _, _ = solver_random(57 + i, find_ranges=bool(i % 2))
        _check_dense(sol, dtype, seed=11 + i)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_elimination_ranges_found_and_given(dtype):
    for i in range(3):
        sol, _, _ = solver_random(57 + i, fill=0.03, elim=(0, 60), ranges=[0, 60])
        assert sol.sparseEliminationRanges().tolist()[:2] == [0, 60]
        _check_dense(sol, dtype, seed=3 + i)
        sol, _, _ = solver_random(61 + i, fill=0.03, elim=(0, 60))
        _check_dense(sol, dtype, seed=7 + i)


def test_given_range_with_lumps_wider_than_the_small_kernels():
    size = 60
    cols = T.make_independent_elim_set(T.random_cols(size, 0.08, 91), 0, 25)
    ss = T.columns_to_structure(cols)
    ps = np.where(np.arange(size) % 5 == 0, 23, 4).astype(np.int64)
    sol = B.create_solver(B.Settings(), ps, ss, [0, 25])
    assert sol.sparseEliminationRanges().tolist()[:2] == [0, 25]
    _check_dense(sol, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_lumps_from_skeleton(dtype):
    """explicit skeletons: one lump of width W (several 64-column blocks, ragged last one) above two
    dense lumps, sparse boards"""
    for W in (5, 64, 65, 300, 515):
        sizes, tot = [], 0
        while tot < W:
            s = min(1 + len(sizes) % 3, W - tot)
            sizes.append(s)
            tot += s
        n0 = len(sizes)
        tail1, tail2 = [3] * 13 + [1], [2] * 15
        sizes = sizes + tail1 + tail2
        span_start = np.concatenate([[0], np.cumsum(sizes)])
        l2s = [0, n0, n0 + len(tail1), n0 + len(tail1) + len(tail2)]
        nspans = len(sizes)
        rows0 = list(range(n0)) + [q for q in range(n0, nspans) if (q * 7 + W) % 5 != 0]
        rows1 = list(range(n0, nspans))
        rows2 = list(range(n0 + len(tail1), nspans))
        col_ptr = np.cumsum([0, len(rows0), len(rows1), len(rows2)])
        sol = B.Solver.from_skeleton(span_start, l2s, col_ptr, rows0 + rows1 + rows2)
        _check_dense(sol, dtype, seed=100 + W)


def test_grid_narrow_root():
    """GRID-like: nested dissection, narrow root lump (the factor's persistent tail)"""
    ss = T.gen_grid(40, 40, 1.0, 2, 37)
    sol = B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)
    _check_dense(sol, np.float64)


def test_meridians_forest():
    """MERI-like: several deep independent roots"""
    ss = T.gen_meridians(4, 150, 0.5, 12, 60, 2, 2, 37)
    sol = B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)
    _check_dense(sol, np.float64)


def test_block_diagonal_forest():
    cols = [[i, i + 1] if i % 7 != 6 and i + 1 < 70 else [i] for i in range(70)]
    ss = T.columns_to_structure(cols)
    sol = B.create_solver(B.Settings(), T.random_vec(70, 2, 5, 3), ss)
    _check_dense(sol, np.float64)


def test_add_fill_for_given_elims_is_refused():
    """AddFillForGivenElims: the solver can only factor up to the range end; a selected inverse
    needs a complete factor and says so"""
    import torch
    sol, _, _ = solver_random(61, fill=0.03, elim=(0, 60), ranges=[0, 60], policy=B.AddFillForGivenElims)
    assert sol.canFactorUpToSpan() < sol.numSpans()
    d = torch.zeros(sol.dataSize(), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="complete factor"):
        sol.selectedInverse(d)


def test_symmetric_bitwise_reproducible_marginals_and_streams():
    """two runs on copies of ONE factor (factor() itself sums with atomics in its elimination
    gather) are bitwise identical, also on a non-default stream"""
    import torch
    sol, ps, _ = solver_random(58, fill=0.05, elim=(0, 40))
    data = spd_data(sol, 9)
    L = to_dev(data)
    sol.factor(L)
    a, b, d = L.clone(), L.clone(), L.clone()
    sol.selectedInverse(a)
    sol.selectedInverse(b)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    sol.setStream(s)
    try:
        with torch.cuda.stream(s):
            sol.selectedInverse(d)
        s.synchronize()
    finally:
        sol.setStream(None)
    assert torch.equal(a, d)
    # diagonal blocks symmetric to the last bit; marginals() = diagBlock reads
    h = a.cpu().numpy()
    blocks = []
    for p in range(len(ps)):
        off, st = sol.diagBlockOffset(p)
        n = int(ps[p])
        blk = np.array([[h[off + i * st + j] for j in range(n)] for i in range(n)])
        assert np.array_equal(blk, blk.T), p
        blocks.append(blk)
    m = sol.marginals(a, list(range(len(ps))))
    assert isinstance(m, list)
    for p in range(len(ps)):
        assert np.array_equal(m[p].cpu().numpy(), blocks[p])
    same = [p for p in range(len(ps)) if ps[p] == ps[0]]
    m = sol.marginals(a, same)
    assert tuple(m.shape) == (len(same), int(ps[0]), int(ps[0]))
    for k, p in enumerate(same):
        assert np.array_equal(m[k].cpu().numpy(), blocks[p])


def _diag_index(sol):
    sk = sol.skel()
    ls = sk["lumpStart"]
    w = (ls[1:] - ls[:-1]).astype(np.int64)
    d0 = sk["chainData"][sk["chainColPtr"][:-1]]
    rep = np.repeat(np.arange(len(w)), w)
    within = np.arange(int(w.sum())) - np.repeat(np.cumsum(w) - w, w)
    return d0[rep] + within * (w[rep] + 1)


def test_bal871_columns_against_solve():
    """full size: Z's blocks in the column of a parameter p equal X of A X = E_p (library solve on an
    untouched copy of the factor), for a few cameras and points"""
    import torch
    num_pts = 527480
    sizes, ss, _, _ = T.gen_bal_synthetic()
    sol = B.create_solver(B.Settings(), sizes, ss, [0, num_pts])
    h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
    h[_diag_index(sol)] = 1.05 * cref.abs_row_sums(sol.skel(), h) + 1e-3
    d = torch.from_numpy(h).cuda()
    sol.factor(d)
    L = d.clone()
    sol.selectedInverse(d)
    torch.cuda.synchronize()
    Z = d.cpu().numpy()
    cams = [num_pts + 3, num_pts + 500]
    pts = [0, 1234, num_pts - 1]
    params = cams + pts
    n = sol.order()
    p2s = sol.paramToSpan()
    sst = sol.skel()["spanStart"]
    cols = []
    for p in params:
        s = int(p2s[p])
        for i in range(int(sst[s]), int(sst[s + 1])):
            e = np.zeros(n)
            e[i] = 1.0
            cols.append(e)
    v = torch.from_numpy(np.concatenate(cols)).cuda()
    sol.solve(L, v, n, len(cols))
    X = v.cpu().numpy().reshape(len(cols), n).T
    # rows of the check: every camera + the points that see the chosen cameras or are chosen
    ptrs, inds = ss.ptrs, ss.inds
    c0 = 0
    checked = 0
    for p in params:
        np_ = int(sizes[p])
        Xp = X[:, c0:c0 + np_]
        c0 += np_
        qs = set(range(num_pts, num_pts + 871, 37)) | set(pts) | set(cams)
        qs |= {int(q) for q in inds[ptrs[p]:ptrs[p + 1]]}
        for q in sorted(qs):
            try:
                off, st, fl = sol.blockOffset(q, p) if q != p else (*sol.diagBlockOffset(p), False)
            except RuntimeError:
                continue
            nq = int(sizes[q])
            sq = int(p2s[q])
            rows = Xp[int(sst[sq]):int(sst[sq]) + nq]
            if fl:
                blk = np.array([[Z[off + i * st + j] for j in range(nq)] for i in range(np_)]).T
            else:
                blk = np.array([[Z[off + i * st + j] for j in range(np_)] for i in range(nq)])
            err = np.abs(blk - rows).max() / np.abs(Xp).max()
            assert err < 1e-10, (p, q, err)
            checked += 1
    assert checked > 3 * len(params)
