"""Host: the plan of the products with the factor (csrc/factor_product_plan.cpp)
against a numpy counting sort of the skeleton's chains, the Lt work lists against the skeleton, the
reference module on a dense example, the exported names and the argument errors of the C entries."""
import ctypes

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import autograd as BA
from baspacho_amd import sparse as S
import factor_product_ref as R
import helpers as H

LONG_TERMS, HUGE_CHAINS, LANE_CHAIN, NARROW, CHUNK_ROWS, STRIP = 128, 256, 16, 8, 256, 64


def _check_plan(sol):
    sk, plan = sol.skel(), sol._testFactorProductPlan()
    nspans, nchains = sol.numSpans(), len(sk["chainRowSpan"])
    ptr, chains, lump = R.counting_sort_plan(sk)
    assert np.array_equal(plan["spanChainPtr"], ptr)
    assert np.array_equal(plan["spanChain"], chains)
    assert np.array_equal(plan["spanChainLump"], lump)
    # every chain once; ascending column lump inside a span; a span without chains has an empty range
    assert np.array_equal(np.sort(plan["spanChain"]), np.arange(nchains))
    count = np.bincount(np.asarray(sk["chainRowSpan"], dtype=np.int64), minlength=nspans)
    for s in range(nspans):
        a, b = int(plan["spanChainPtr"][s]), int(plan["spanChainPtr"][s + 1])
        assert b - a == count[s]
        assert np.all(np.diff(plan["spanChainLump"][a:b]) > 0)
        assert np.all(np.asarray(sk["chainRowSpan"])[plan["spanChain"][a:b]] == s)
    # the kind of a span, from the stored terms of its last row: one lane per row, one wave per row above
    # LONG_TERMS, and of those the span per workgroup when it has at most 64 rows and at least HUGE_CHAINS
    # chains of lumps of at most LANE_CHAIN columns
    t = R.stored_lower(sol).sum(1)
    ss = np.asarray(sk["spanStart"], dtype=np.int64)
    lw = np.diff(np.asarray(sk["lumpStart"], dtype=np.int64))
    narrow = np.array([(lw[plan["spanChainLump"][plan["spanChainPtr"][s]:plan["spanChainPtr"][s + 1]]] <= LANE_CHAIN).sum()
                       for s in range(nspans)])
    last = t[ss[1:] - 1]
    kind = np.where((last > LONG_TERMS) & (narrow >= HUGE_CHAINS) & (np.diff(ss) <= 64), 2,
                    (last > LONG_TERMS).astype(np.int64))
    assert np.array_equal(plan["spanLong"], kind)
    long_rows = np.concatenate([np.arange(ss[s], ss[s + 1]) for s in range(nspans) if kind[s] == 1] or
                               [np.zeros(0, dtype=np.int64)])
    assert np.array_equal(plan["longRows"], long_rows)
    assert np.array_equal(plan["hugeSpans"], np.nonzero(kind == 2)[0])
    ls_ = np.asarray(sk["lumpStart"], dtype=np.int64)
    wide = []
    for k, s in enumerate(plan["hugeSpans"]):
        assert plan["hugeWidePtr"][k] == len(wide)
        a, b = int(plan["spanChainPtr"][s]), int(plan["spanChainPtr"][s + 1])
        lumps = plan["spanChainLump"][a:b]
        wide += (a + np.nonzero(ls_[lumps + 1] - ls_[lumps] > LANE_CHAIN)[0]).tolist()
    assert plan["hugeWidePtr"][-1] == len(wide) and plan["hugeWide"].tolist() == wide
    # y = L^T x: every column is a packed column of a narrow lump or a column of exactly one strip, and
    # the chunks of a strip tile its rows from the strip's first column to the end of the lump
    ls = np.asarray(sk["lumpStart"], dtype=np.int64)
    ccp, till = np.asarray(sk["chainColPtr"]), np.asarray(sk["chainRowsTillEnd"])
    owner = np.zeros(sol.order(), dtype=np.int64)
    np.add.at(owner, plan["smallCol"], 1)
    assert np.all(ls[1:][plan["smallColLump"]] - ls[plan["smallColLump"]] <= NARROW)
    assert np.all((ls[plan["smallColLump"]] <= plan["smallCol"]) & (plan["smallCol"] < ls[1:][plan["smallColLump"]]))
    tk = plan["tasks"]
    strips = {}
    for i in range(len(tk["lump"])):
        l, c0, nc, w = (int(tk[f][i]) for f in ("lump", "c0", "nc", "w"))
        assert w == ls[l + 1] - ls[l] > NARROW and c0 % STRIP == 0 and nc == min(STRIP, w - c0)
        assert tk["dataOff"][i] == sk["chainData"][ccp[l]]
        c = int(tk["chain"][i])
        assert ccp[l] <= c < ccp[l + 1]
        if tk["rBeg"][i] < tk["rEnd"][i]:
            assert (0 if c == ccp[l] else till[c - 1]) <= tk["rBeg"][i] < till[c]
        strips.setdefault((l, c0), []).append(i)
    parts = []
    for (l, c0), idx in strips.items():
        R_l = int(till[ccp[l + 1] - 1])
        owner[ls[l] + c0:ls[l] + c0 + int(tk["nc"][idx[0]])] += 1
        assert tk["rBeg"][idx[0]] == c0 and tk["rEnd"][idx[-1]] == R_l
        assert np.array_equal(tk["rEnd"][idx[:-1]], tk["rBeg"][idx[1:]])
        assert len(idx) == max(1, -(-(R_l - c0) // CHUNK_ROWS))
        if len(idx) == 1:
            assert tk["part"][idx[0]] == -1
        else:
            parts.append((int(ls[l] + c0), int(tk["nc"][idx[0]]), int(tk["part"][idx[0]]), len(idx)))
            assert np.array_equal(tk["part"][idx], tk["part"][idx[0]] + STRIP * np.arange(len(idx)))
    assert np.all(owner == 1)
    fd = plan["folds"]
    assert sorted(parts) == sorted(zip(*(fd[f].tolist() for f in ("col0", "nc", "part0", "numChunks"))))
    at = 0  # the partial sums of the split strips tile [0, partElems)
    for p in sorted(parts, key=lambda p: p[2]):
        assert p[2] == at
        at += STRIP * p[3]
    assert plan["partElems"] == at


@pytest.mark.parametrize("name", R.structure_names())
def test_plan_is_the_counting_sort_of_the_chains(name):
    _check_plan(R.solver(name))


@pytest.mark.parametrize("elim", [None, (0, 60)])
@pytest.mark.parametrize("seed", [3, 11])
def test_plan_on_random_structures(seed, elim):
    sol, _, _ = H.solver_random(seed, elim=elim, ranges=() if elim is None else list(elim))
    _check_plan(sol)


def test_structures_cover_the_kernel_paths():
    """the test structures reach every path: long and short spans, more than 64 chains in one span, packed
    narrow lumps, strips of one chunk and split strips, ragged strips"""
    bal = R.solver("bal")._testFactorProductPlan()
    assert set(bal["spanLong"].tolist()) == {0, 1} and len(bal["smallCol"]) >= 3 * 150
    assert np.diff(bal["spanChainPtr"]).max() > 64
    # huge spans: two fed by more than 16 groups of 7 narrow chains and one wide chain (the camera lump); a span
    # of more than 64 rows with as many narrow chains stays with the rows per wave
    huge = R.solver("bal_huge")._testFactorProductPlan()
    assert len(huge["hugeSpans"]) == 2 and np.diff(huge["hugeWidePtr"]).tolist() == [1, 1]
    assert np.diff(huge["spanChainPtr"])[huge["hugeSpans"]].min() > 16 * 7
    tall = R.solver("bal_tall")._testFactorProductPlan()
    assert len(tall["hugeSpans"]) == 0 and tall["spanLong"][-1] == 1 and len(tall["longRows"]) == 70
    assert np.diff(tall["spanChainPtr"])[-1] > HUGE_CHAINS
    d257 = R.solver("dense257")._testFactorProductPlan()
    assert len(d257["folds"]["col0"]) >= 1 and (d257["tasks"]["part"] == -1).any() and (d257["tasks"]["nc"] == 1).any()
    assert len(R.solver("dense1")._testFactorProductPlan()["smallCol"]) == 1
    assert R.solver("splitk2049")._testFactorProductPlan()["partElems"] > 0


def test_reference_is_self_consistent_on_a_dense_example():
    sol = R.solver("dense64")
    data, x = R.random_operands(sol, np.float64, 3, seed=1)
    Ld = R.dense_lower(sol, data)
    assert np.isfinite(Ld).all() and np.array_equal(Ld, np.tril(Ld))
    for transposed in (False, True):
        M = Ld.T if transposed else Ld
        ref, t, s = R.reference(sol, data, x, transposed)
        assert ref.dtype == np.longdouble and ref.shape == (64, 3)
        assert np.array_equal(t, np.arange(64, 0, -1) if transposed else np.arange(1, 65))
        assert np.allclose(ref.astype(np.float64), M @ x, rtol=0, atol=1e-13)
        assert np.allclose(s, np.abs(M) @ np.abs(x), rtol=1e-14, atol=0)
        R.check(sol, data, x, M @ x, transposed)
        wrong = (M @ x).copy()
        wrong[5, 1] += 4 * R.bound(t, s, np.float64)[5, 1]
        with pytest.raises(AssertionError):
            R.check(sol, data, x, wrong, transposed)
        with pytest.raises(AssertionError):
            R.check(sol, data, x, np.where(np.arange(64)[:, None] == 7, np.nan, M @ x), transposed)
    ref32, _, _ = R.reference(sol, data.astype(np.float32), x.astype(np.float32), False)
    assert ref32.dtype == np.float64


def test_names_are_exported():
    for name in ("mulL", "mulLt", "_testFactorProductPlan"):
        assert callable(getattr(B.Solver, name))
    assert "mul_l" in BA.__all__ and "mul_lt" in BA.__all__ and callable(BA.mul_l) and callable(BA.mul_lt)
    assert "whiten" in S.__all__ and "sample_cov" in S.__all__ and callable(S.whiten) and callable(S.sample_cov)
    assert "S.whiten(" in S.__doc__ and "S.sample_cov(" in S.__doc__
    lib = R.solver("dense1")._lib
    for base in ("bsp_factor_product", "bsp_factor_product_batched"):
        for sfx in ("_f64", "_f32"):
            assert hasattr(lib, base + sfx)
    assert hasattr(lib, "bsp_test_factor_product_plan")


def test_argument_errors_launch_nothing():
    """in == out or overlapping ranges, nrhs < 1, a stride below order(), a bad `which`, NULL pointers and an
    empty batch: an error from the argument checks, which run before any device work (fake addresses)"""
    sol = R.solver("tridiag")
    n, lib = sol.order(), sol._lib
    L, X, Y = 1 << 30, 1 << 31, 1 << 32  # never dereferenced
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32

    def single(fn, l, which, x, ldx, y, ldy, k):
        return fn(sol._h, vp(l), i32(which), vp(x), i64(ldx), vp(y), i64(ldy), i32(k))

    for fn, size in ((lib.bsp_factor_product_f64, 8), (lib.bsp_factor_product_f32, 4)):
        for which in (0, 1):
            for args, word in [((L, which, X, n, X, n, 1), "overlaps"),
                               ((L, which, X, n, X + size * (n - 1), n, 1), "overlaps"),
                               ((L, which, X, n + 2, X + size * (n + 1), n + 2, 2), "overlaps"),
                               ((L, which, X, n, L + size * (sol.dataSize() - 1), n, 1), "overlaps"),
                               ((L, which, X, n, Y, n, 0), "nRHS"), ((L, which, X, n, Y, n, -3), "nRHS"),
                               ((L, which, X, n - 1, Y, n, 1), "stride"), ((L, which, X, n, Y, n - 1, 2), "stride"),
                               ((None, which, X, n, Y, n, 1), "NULL"), ((L, which, None, n, Y, n, 1), "NULL"),
                               ((L, which, X, n, None, n, 1), "NULL")]:
                assert single(fn, *args) != 0, args
                assert word in lib.bsp_last_error().decode(), (args, lib.bsp_last_error())
        assert single(fn, L, 2, X, n, Y, n, 1) != 0 and "which" in lib.bsp_last_error().decode()
        assert single(fn, L, -1, X, n, Y, n, 1) != 0 and "which" in lib.bsp_last_error().decode()

    def ptrs(*a):
        return (ctypes.c_void_p * len(a))(*a)

    for fn, size in ((lib.bsp_factor_product_batched_f64, 8), (lib.bsp_factor_product_batched_f32, 4)):
        def batched(ls, which, xs, ldx, ys, ldy, k, batch):
            return fn(sol._h, ls, i32(which), xs, i64(ldx), ys, i64(ldy), i32(k), i32(batch))
        two = size * n
        assert batched(ptrs(L, L), 1, ptrs(X, X + two), n, ptrs(Y, Y + two - size), n, 1, 2) != 0
        assert "overlap" in lib.bsp_last_error().decode()
        assert batched(ptrs(L, L), 0, ptrs(X, X + two), n, ptrs(Y, X + two), n, 1, 2) != 0
        assert "overlaps" in lib.bsp_last_error().decode()
        assert batched(ptrs(L), 0, ptrs(X), n, ptrs(Y), n, 1, 0) != 0 and "empty" in lib.bsp_last_error().decode()
        assert batched(None, 0, ptrs(X), n, ptrs(Y), n, 1, 1) != 0 and "NULL" in lib.bsp_last_error().decode()
        assert batched(ptrs(L, None), 0, ptrs(X, X + two), n, ptrs(Y, Y + two), n, 1, 2) != 0
        assert "NULL" in lib.bsp_last_error().decode()
        assert batched(ptrs(L, L), 0, ptrs(X, X + two), n, ptrs(Y, Y + two), n, 0, 2) != 0
        assert "nRHS" in lib.bsp_last_error().decode()
