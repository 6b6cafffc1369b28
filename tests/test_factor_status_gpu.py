"""GPU: the factor status, the damping of the diagonal and the regularised retry (DESIGN.md section 18;
csrc/hip_status_kernels.h) against the numpy restatement of tests/factor_status_ref.py.

1. the scan on arbitrary framed, poisoned buffers: all four words exact, nothing but the record written;
2. the status after factor(), kernel path by kernel path: a negative pivot planted at internal scalar k
   gives w[0] == k (tests/test_factor_status_cpu.py fixes that the planted inputs have that one answer);
3. dampDiagonal bitwise against the restatement;
4. factorRegularized on a matrix whose smallest eigenvalue is known;
5. sparse.check_positive_definite in the caller's order."""
import ctypes

import numpy as np
import pytest

import baspacho_amd as B
import factor_status_ref as R
from buffer_edges import Frame, SENTINEL_BITS, bitwise_equal, framed, poison_upper
from helpers import solver_random, spd_data, to_dev
from kf_structures import bipartite, counter_delta, dense_solver, lump_over_lump, random_with_range

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def _torch_dtype(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _words(t):
    return t.cpu().numpy().astype(np.int64)


# ---- 1. the scan against the restatement on arbitrary buffers ---------------------------------------

def _arbitrary(sol, seed, dtype):
    """random data with a positive diagonal, the sentinel NaN in the strictly-upper elements"""
    rng = np.random.default_rng(seed)
    data = rng.uniform(-1.0, 1.0, sol.dataSize()).astype(dtype)
    data[sol.diagOffsets()] = rng.uniform(0.5, 2.0, sol.order()).astype(dtype)
    return poison_upper(data, sol)


def _scan_scalars(sol):
    """0, the last, both sides of the 2048-element workgroup boundary, the first and last of a lump"""
    n, ls = sol.order(), sol.skel()["lumpStart"]
    mid = sol.numLumps() // 2
    ks = [0, n - 1, int(ls[mid]), int(ls[mid + 1]) - 1] + [k for k in (2047, 2048, 2049) if k < n]
    return sorted(set(ks))


def _scan_ranges(sol):
    """all spans, a range that starts and ends inside a lump, one that starts inside the first lump and
    ends inside the last, and an empty one"""
    sk, ns = sol.skel(), sol.numSpans()
    l2s = sk["lumpToSpan"]
    wide = int(np.argmax(np.diff(l2s)))  # the lump of most spans
    inside = (int(l2s[wide]) + 1, int(l2s[wide + 1]) - 1) if l2s[wide + 1] - l2s[wide] >= 3 else (1, ns - 1)
    return [(0, ns), inside, (1, ns - 1), (ns // 2, ns // 2), (ns, ns)]


SCAN_STRUCTURES = {
    "random_400": lambda: solver_random(57)[0],                  # order below 2048, many lumps
    "dense_2048": lambda: dense_solver(2048),                    # exactly one full workgroup
    "two_lumps_2060": lambda: lump_over_lump(1400, 660),         # above: 2047 / 2048 / 2049 in the second lump
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SCAN_STRUCTURES))
def test_scan_matches_the_restatement_on_framed_poisoned_buffers(name, dtype):
    import torch
    sol = SCAN_STRUCTURES[name]()
    n, diag = sol.order(), sol.diagOffsets()
    assert {"random_400": n < 2048, "dense_2048": n == 2048, "two_lumps_2060": n > 2049}[name], n
    base = _arbitrary(sol, 5, dtype)
    ks = _scan_scalars(sol)
    tiny = np.finfo(dtype).smallest_subnormal
    plants = [np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, tiny]
    cases = [("clean", base)]
    for v in plants:  # the value at every chosen scalar
        d = base.copy()
        d[diag[ks]] = dtype(v)
        cases.append((repr(v), d))
    for i, k in enumerate(ks):  # one scalar at a time, the values in turn
        d = base.copy()
        d[diag[k]] = dtype(plants[i % 6])
        cases.append(("one bad at %d" % k, d))
    d = base.copy()  # half of the diagonals bad
    d[diag] = np.random.default_rng(9).uniform(-1.0, 1.0, n).astype(dtype)
    cases.append(("random signs", d))
    fr = Frame([sol.dataSize()], dtype)
    for what, d in cases:
        fr.fill(0, d).seal()
        for b, e in _scan_ranges(sol):
            got = _words(sol.factorStatus(fr.view(0), b, e))
            want = R.scan(sol, d, b, e)
            assert np.array_equal(got, want), (name, what, (b, e), got, want)
        fr.assert_intact(read_only=[0], what=(name, what))
    # the denormal counts as good and is the minimum; the sentinel in the upper elements never counted
    d = base.copy()
    d[diag[ks[-1]]] = tiny
    fr.fill(0, d).seal()
    first, count, mn, mx = R.decode(_words(sol.factorStatus(fr.view(0))))
    assert (first, count, mn) == (-1, 0, float(tiny)) and mx == float(d[diag].max())
    # nothing but the four words of dev_out is written
    lib = sol._lib
    out = torch.full((12,), -77, dtype=torch.int64, device="cuda")
    rc = getattr(lib, "bsp_factor_status_" + ("f64" if dtype == np.float64 else "f32"))(
        sol._h, ctypes.c_void_p(fr.view(0).data_ptr()), ctypes.c_int64(0), ctypes.c_int64(sol.numSpans()),
        ctypes.c_void_p(out.data_ptr() + 32))
    assert rc == 0, lib.bsp_last_error()
    got = _words(out)
    assert np.array_equal(got[4:8], R.scan(sol, d)) and (got[:4] == -77).all() and (got[8:] == -77).all()
    fr.assert_intact(read_only=[0], what=(name, "raw call"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_batch_across_the_member_chunk_limit_is_bitwise_the_single_call(dtype):
    """65537 members (logDet's chunk is 65535) on a tiny structure: views of one tensor of 7 rows"""
    import torch
    sol = dense_solver(24)
    rows, batch = 7, 65537
    host = np.stack([_arbitrary(sol, 20 + r, dtype) for r in range(rows)])
    diag = sol.diagOffsets()
    for r, v in enumerate([np.nan, -1.0, 0.0, np.inf, 1.0, -0.0, 2.5]):
        host[r, diag[(5 * r) % sol.order()]] = v
    dev = to_dev(host)
    singles = np.stack([_words(sol.factorStatus(dev[r])) for r in range(rows)])
    for r in range(rows):
        assert np.array_equal(singles[r], R.scan(sol, host[r])), r
    assert len({tuple(s) for s in singles}) == rows  # the members differ
    got = _words(sol.factorStatus([dev[q % rows] for q in range(batch)]))
    assert got.shape == (batch, 4)
    assert np.array_equal(got, singles[np.arange(batch) % rows])
    # a sub-range and the decoded list
    part = _words(sol.factorStatus([dev[r] for r in range(rows)], 1, 2))
    for r in range(rows):
        assert np.array_equal(part[r], R.scan(sol, host[r], 1, 2)), r
    st = sol.readFactorStatus(sol.factorStatus([dev[0], dev[4]]))
    assert [s["ok"] for s in st] == [False, True] and st[0]["first"] == 0 and st[0]["param"] is not None


# ---- 2. the status after factor(), per kernel path ---------------------------------------------------

def _factor_status(sol, host, factor=None, span_range=(0, None)):
    dev = to_dev(host)
    (factor or sol.factor)(dev)
    st = sol.readFactorStatus(sol.factorStatus(dev, *span_range))
    return st, dev


def _assert_first_is(sol, data, k, what, factor=None, span_range=(0, None)):
    """plants the negative pivot at internal scalar k, factors, and asserts the contract of w[0]"""
    st, dev = _factor_status(sol, R.plant_negative(sol, data, k), factor, span_range)
    print(what, "k = %d:" % k, st)
    assert st["first"] == k and st["count"] >= 1 and not st["ok"] and st["minDiag"] > 0, (what, k, st)
    ss, p2s = sol.skel()["spanStart"], sol.paramToSpan()
    span = int(p2s[st["param"]])
    assert int(ss[span]) + st["offsetInParam"] == k and k < int(ss[span + 1])
    return st, dev


def _assert_clean(sol, data, what):
    st, dev = _factor_status(sol, data)
    d = dev.cpu().numpy()[sol.diagOffsets()].astype(np.float64)
    assert st["ok"] and st["count"] == 0 and st["first"] == -1 and st["param"] is None, (what, st)
    assert st["minDiag"] == d.min() and st["maxDiag"] == d.max(), (what, st, d.min(), d.max())


def _lump_of(sol, k):
    return int(np.searchsorted(sol.skel()["lumpStart"], k, side="right")) - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_after_factor_sparse_elimination_lump(dtype):
    sol = bipartite(300, 12, 3, 6, seed=4)
    data = spd_data(sol, 21, dtype=dtype)
    _assert_clean(sol, data, "bipartite")
    er = sol.sparseEliminationRanges()
    for k in (0, 3 * 100 + 1, 3 * 299 + 2):  # inside point blocks
        assert _lump_of(sol, k) < int(er[-1]), "k is not in the sparse-elimination range"
        _assert_first_is(sol, data, k, "point block")
    for k in (900, 900 + 31, sol.order() - 1):  # the cameras behind the points, the last scalar
        assert _lump_of(sol, k) >= int(er[-1])
        _assert_first_is(sol, data, k, "cameras")


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_after_factor_small_tree_lumps(dtype):
    sol, _, _ = solver_random(57)
    data = spd_data(sol, 22, dtype=dtype)
    _assert_clean(sol, data, "solver_random")
    ls = sol.skel()["lumpStart"]
    mid = sol.numLumps() // 2
    # a tree of lumps narrower than a panel below a wider root, none of them eliminated sparsely
    assert sol.numLumps() > 8 and 1 < ls[mid + 1] - ls[mid] < 64 and len(sol.sparseEliminationRanges()) == 0
    for k in (int(ls[mid]), int(ls[mid + 1]) - 1, int(ls[1]) - 1, int(ls[-2]), sol.order() - 1):
        _assert_first_is(sol, data, k, "tree lump")


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_after_factor_dense_lump_of_200(dtype):
    sol = dense_solver(200)
    assert sol.numLumps() == 1
    data = spd_data(sol, 23, dtype=dtype)
    _assert_clean(sol, data, "dense 200")
    for k in (64, 64 + 31, 64 + 63, 128, 197, 199):  # k % 64 in {0, 31, 63}; the ragged last panel; the last scalar
        _assert_first_is(sol, data, k, "dense lump")


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_after_factor_lump_over_lump(dtype):
    sol = lump_over_lump(200, 130)
    data = spd_data(sol, 24, dtype=dtype)
    _assert_clean(sol, data, "lump over lump")
    for k in (200, 200 + 70, 329):  # in the lower lump
        assert _lump_of(sol, k) == 1
        _assert_first_is(sol, data, k, "lower lump")
    _assert_first_is(sol, data, 130, "upper lump")


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_after_factor_persistent_tail(monkeypatch, dtype):
    """the exchange slots of the tail are polled as data against an all-ones arm word and all-ones
    results are canonicalised when published (csrc/hip_sweep_kernels.h, sweepPublish / sweepValid): the
    NaN of a failed pivot is an ordinary value to them"""
    monkeypatch.setenv("BSP_TAIL_BLOCKS", "4")
    sol = dense_solver(1536)
    tail_start = sol.order() - 64 * sol.planStats()["num_tail_panels"]  # the tail: whole panels up to the last column
    data = spd_data(sol, 25, dtype=dtype)
    k = 1536 - 3 * 256 + 64 + 12  # in the second panel of the tail's second outer block
    assert 0 < tail_start == 1536 - 4 * 256 and tail_start + 64 <= k < sol.order(), "k is not in a tail panel"
    assert counter_delta(sol, "tail_launches", lambda: _assert_first_is(sol, data, k, "persistent tail")) == 1, \
        "the persistent tail was not the path taken"
    assert counter_delta(sol, "tail_launches", lambda: _assert_clean(sol, data, "dense 1536")) == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_of_a_batch_with_one_broken_member(dtype):
    sol = lump_over_lump(200, 130)
    hosts = [spd_data(sol, 30 + q, dtype=dtype) for q in range(3)]
    k = 200 + 17
    hosts[1] = R.plant_negative(sol, hosts[1], k)
    devs = [to_dev(h) for h in hosts]
    sol.factor(devs)
    st = sol.readFactorStatus(sol.factorStatus(devs))
    print(st)
    assert [s["ok"] for s in st] == [True, False, True]
    assert st[1]["first"] == k and st[1]["count"] >= 1 and st[1]["minDiag"] > 0
    for q in (0, 2):
        d = devs[q].cpu().numpy()[sol.diagOffsets()].astype(np.float64)
        assert (st[q]["minDiag"], st[q]["maxDiag"]) == (d.min(), d.max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_of_an_exactly_zero_first_pivot(dtype):
    for sol in (dense_solver(200), bipartite(300, 12, 3, 6, seed=4), solver_random(57)[0]):
        data = spd_data(sol, 26, dtype=dtype)
        data[sol.diagOffsets()[0]] = 0
        st, _ = _factor_status(sol, data)
        print(st)
        assert st["first"] == 0 and st["count"] >= 1 and not st["ok"] and st["offsetInParam"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_of_partial_factors(dtype):
    for sol in (lump_over_lump(200, 130), random_with_range(5)):
        sk, ns = sol.skel(), sol.numSpans()
        er = sol.sparseEliminationRanges()
        lump = max(int(er[-1]) if len(er) else 0, 1) + (sol.numLumps() > 3)
        span, bar = int(sk["lumpToSpan"][lump]), int(sk["lumpStart"][lump])
        data = spd_data(sol, 27, dtype=dtype)
        # factorUpTo(span), range [0, span): a pivot before the cut
        k = bar - 2
        _assert_first_is(sol, data, k, "factorUpTo", lambda d: sol.factorUpTo(d, span), (0, span))
        # a pivot behind the cut: the leading columns are clean, factorFrom(span) then breaks at k
        k = bar + 3
        st, dev = _factor_status(sol, R.plant_negative(sol, data, k), lambda d: sol.factorUpTo(d, span), (0, span))
        assert st["ok"] and st["count"] == 0, st
        sol.factorFrom(dev, span)
        st = sol.readFactorStatus(sol.factorStatus(dev, span, ns))
        print("factorFrom k = %d:" % k, st)
        assert st["first"] == k and st["count"] >= 1 and st["minDiag"] > 0, st
        # unplanted: both ranges clean, min and max those of their part of the diagonal
        dev = to_dev(data)
        sol.factorUpTo(dev, span)
        a = sol.readFactorStatus(sol.factorStatus(dev, 0, span))
        sol.factorFrom(dev, span)
        b = sol.readFactorStatus(sol.factorStatus(dev, span, ns))
        d = dev.cpu().numpy()[sol.diagOffsets()].astype(np.float64)
        assert a["ok"] and (a["minDiag"], a["maxDiag"]) == (d[:bar].min(), d[:bar].max())
        assert b["ok"] and (b["minDiag"], b["maxDiag"]) == (d[bar:].min(), d[bar:].max())


# ---- 3. dampDiagonal ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_damp_is_bitwise_the_restatement(dtype):
    import torch
    for sol in (solver_random(57)[0], lump_over_lump(1400, 660)):
        ns = sol.numSpans()
        data = poison_upper(spd_data(sol, 41, dtype=dtype), sol)
        l2s = sol.skel()["lumpToSpan"]
        wide = int(np.argmax(np.diff(l2s)))
        inside = (int(l2s[wide]) + 1, int(l2s[wide + 1]) - 1)  # starts and ends inside a lump
        for (b, e), (alpha, beta) in (((0, ns), (0.125, 3.0)), (inside, (1e-3, 0.3)), ((1, ns - 1), (-0.5, 1e-7)),
                                      ((ns // 2, ns // 2), (1.0, 1.0)), ((0, ns), (0.0, 0.0))):
            fr = framed(dtype, [data])
            sol.dampDiagonal(fr.view(0), alpha, beta, b, e)
            want = R.damp(sol, data, alpha, beta, b, e)
            # every word: the diagonals of the range, every off-diagonal element, the poisoned upper ones
            assert bitwise_equal(fr.host(0), want), (sol.order(), (b, e), alpha, beta)
            fr.assert_intact(what=("damp", (b, e)))
        if dtype == np.float64:  # the host Solver.damp on the full range
            dev = to_dev(data)
            sol.dampDiagonal(dev, 0.25, 7.0)
            assert bitwise_equal(dev.cpu().numpy(), sol.damp(data.copy(), 0.25, 7.0))
        # alpha and beta as device tensors
        dev = to_dev(data)
        ab = torch.tensor([0.375, 2.0], dtype=_torch_dtype(dtype), device="cuda")
        sol.dampDiagonal(dev, ab[0], ab[1])
        assert bitwise_equal(dev.cpu().numpy(), R.damp(sol, data, 0.375, 2.0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_damp_of_a_batch_with_its_own_alpha_and_beta_per_member(dtype):
    import torch
    sol, _, _ = solver_random(57)
    ns, nb = sol.numSpans(), 5
    hosts = [poison_upper(spd_data(sol, 50 + q, dtype=dtype), sol) for q in range(nb)]
    alphas = np.array([0.0, 0.5, 1e-3, -0.25, 2.0], dtype=dtype)
    betas = np.array([1.0, 0.0, 1e-4, 3.5, -1.0], dtype=dtype)
    fr = framed(dtype, hosts)
    sol.dampDiagonal(fr.views(), to_dev(alphas), to_dev(betas), 2, ns - 3)
    for q in range(nb):
        assert bitwise_equal(fr.host(q), R.damp(sol, hosts[q], alphas[q], betas[q], 2, ns - 3)), q
    fr.assert_intact(what="batched damp")
    # one float for all members; members that share a buffer are refused
    devs = [to_dev(h) for h in hosts]
    sol.dampDiagonal(devs, 0.5, torch.tensor(2.0, dtype=_torch_dtype(dtype), device="cuda"))
    for q in range(nb):
        assert bitwise_equal(devs[q].cpu().numpy(), R.damp(sol, hosts[q], 0.5, 2.0)), q
    with pytest.raises(RuntimeError, match="overlap"):
        sol.dampDiagonal([devs[0], devs[0]], 0.0, 1.0)


# ---- 4. factorRegularized ----------------------------------------------------------------------------

def _indefinite(sol, seed, dtype):
    """(A, B, delta): B = spd_data, A = B - (lambda_min(B) + delta) I, delta = 1e-3 max diag(B)"""
    Bd = spd_data(sol, seed, dtype=dtype)
    diag = sol.diagOffsets()
    lam = np.linalg.eigvalsh(sol.densify(Bd.astype(np.float64), fill_upper_half=True))[0]
    delta = 1e-3 * float(Bd[diag].max())
    A = Bd.copy()
    A[diag] = (Bd[diag].astype(np.float64) - (lam + delta)).astype(dtype)
    return A, Bd, delta


@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_regularized_takes_exactly_three_retries(dtype):
    sol, _, _ = solver_random(57, size=60)
    n = sol.order()
    assert n <= 300
    A, _, delta = _indefinite(sol, 61, dtype)
    dev = to_dev(A)
    out, info = sol.factorRegularized(dev, alpha=0.0, beta0=delta / 30, growth=10.0)
    print(info)
    # retries delta/30, delta/3 (leaves an eigenvalue of -2 delta/3: fails), 3.33 delta (+2.33 delta: passes)
    assert info["retries"] == 3 and info["status"]["ok"] and info["alpha"] == 0.0
    assert abs(info["beta"] - delta / 30 * 100) <= 1e-12 * delta
    assert bitwise_equal(dev.cpu().numpy(), A), "A was written"
    damped = R.damp(sol, A, 0.0, dtype(info["beta"]))
    rhs = np.random.default_rng(7).standard_normal(n).astype(dtype)
    v = to_dev(rhs)
    sol.solve(out, v, n, 1)
    X = np.linalg.solve(sol.densify(damped.astype(np.float64), fill_upper_half=True), rhs.astype(np.float64))
    err = np.linalg.norm(v.cpu().numpy().astype(np.float64) - X) / np.linalg.norm(X)
    print("solve error", err)
    assert err < (1e-10 if dtype == np.float64 else 1e-3), err
    # the retries run out
    with pytest.raises(B.FactorizationError) as ei:
        sol.factorRegularized(dev, alpha=0.0, beta0=delta / 30, growth=10.0, maxRetries=1)
    st = ei.value.status
    assert not st["ok"] and st["count"] >= 1 and 0 <= st["first"] < n
    sizes = np.diff(sol.skel()["spanStart"])[sol.paramToSpan()]
    assert 0 <= st["param"] < len(sizes) and 0 <= st["offsetInParam"] < sizes[st["param"]]
    assert bitwise_equal(dev.cpu().numpy(), A)


@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_regularized_retries_only_the_failed_members(dtype):
    sol = lump_over_lump(40, 50)  # one panel per lump: no accumulation whose order could differ between two runs
    A, Bd, delta = _indefinite(sol, 62, dtype)
    members = [to_dev(Bd), to_dev(A)]
    outs, infos = sol.factorRegularized(members, alpha=0.0, beta0=delta / 30, growth=10.0)
    print(infos)
    assert [i["retries"] for i in infos] == [0, 3] and all(i["status"]["ok"] for i in infos)
    assert infos[0]["beta"] == 0.0
    plain = [to_dev(Bd), to_dev(A)]
    sol.factor(plain)
    assert bitwise_equal(outs[0].cpu().numpy(), plain[0].cpu().numpy()), "a member that passed was touched again"
    assert bitwise_equal(members[0].cpu().numpy(), Bd) and bitwise_equal(members[1].cpu().numpy(), A)
    # out given by the caller
    given = [to_dev(np.zeros_like(A)) for _ in range(2)]
    outs2, infos2 = sol.factorRegularized(members, out=given, beta0=delta / 30)
    assert outs2 is given and [i["retries"] for i in infos2] == [0, 3]
    assert bitwise_equal(given[0].cpu().numpy(), plain[0].cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_regularized_default_beta0_leaves_an_spd_matrix_alone(dtype):
    sol, _, _ = solver_random(57, size=60)
    data = spd_data(sol, 63, dtype=dtype)
    dev = to_dev(data)
    out, info = sol.factorRegularized(dev)
    assert info["retries"] == 0 and info["status"]["ok"] and info["beta"] == 0.0
    plain = to_dev(data)
    sol.factor(plain)
    got, want = out.cpu().numpy(), plain.cpu().numpy()
    mask = sol.lowerMask()
    assert np.linalg.norm((got - want)[mask]) <= (1e-12 if dtype == np.float64 else 1e-5) * np.linalg.norm(want[mask])
    # the default comes from the status of the unfactored matrix: 8 eps maxDiag(A)
    st = sol.readFactorStatus(sol.factorStatus(dev))
    assert st["ok"] and st["maxDiag"] == float(data[sol.diagOffsets()].max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_solver_on_a_side_stream(dtype):
    """the Python methods put their own device work (the alpha / beta pairs, the copies of the retry loop,
    the read of the record) on the solver's stream, whatever torch's current stream is"""
    import torch
    sol, _, _ = solver_random(57, size=60)
    A, _, delta = _indefinite(sol, 61, dtype)
    data = spd_data(sol, 64, dtype=dtype)
    dev, devA = to_dev(data), to_dev(A)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    sol.setStream(side)
    try:
        assert torch.cuda.current_stream() != side
        sol.dampDiagonal(dev, 0.375, 2.0)
        st = sol.readFactorStatus(sol.factorStatus(dev))
        out, info = sol.factorRegularized(devA, beta0=delta / 30)
        side.synchronize()
    finally:
        sol.setStream(None)
    want = R.damp(sol, data, 0.375, 2.0)
    assert bitwise_equal(dev.cpu().numpy(), want)
    assert np.array_equal(R.scan(sol, want), [st["first"], st["count"]] + list(
        np.array([st["minDiag"], st["maxDiag"]]).view(np.int64)))
    assert info["retries"] == 3 and info["status"]["ok"] and bitwise_equal(devA.cpu().numpy(), A)


# ---- 5. sparse.check_positive_definite ----------------------------------------------------------------

def _symmetric_problem(n, seed):
    rng = np.random.default_rng(seed)
    pairs = {(i, i) for i in range(n)} | {(i, i - 1) for i in range(1, n)}
    while len(pairs) < 4 * n:
        i, j = sorted(rng.integers(0, n, 2))
        pairs.add((int(j), int(i)))
    rows, cols = (np.array(x, dtype=np.int64) for x in zip(*sorted(pairs)))
    vals = np.where(rows == cols, 10.0 + rng.uniform(0, 1, len(rows)), rng.uniform(-1, 1, len(rows)))
    return rows, cols, vals


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_positive_definite_names_the_callers_scalar(dtype):
    import torch
    from baspacho_amd import sparse as S
    n = 40
    rows, cols, vals = _symmetric_problem(n, 3)
    pat = S.SymmetricPattern(rows, cols, n)
    sol = pat.solver
    perm = sol.scalarPermutation()  # perm[user] = internal
    st = S.check_positive_definite(pat, to_dev(vals.astype(dtype)))
    assert st["ok"] and st["scalar"] is None and st["count"] == 0
    ls = sol.skel()["lumpStart"]
    for k in (0, int(ls[sol.numLumps() // 2]), n - 1):  # internal scalars, as in the per-path cases
        c = int(np.nonzero(perm == k)[0][0])
        v = vals.copy()
        at = int(np.nonzero((rows == c) & (cols == c))[0][0])
        v[at] = -abs(v[at]) - 1
        st = S.check_positive_definite(pat, to_dev(v.astype(dtype)))
        print(k, c, st)
        assert not st["ok"] and st["first"] == k and st["scalar"] == c and st["param"] == c
    # a batch: only the second matrix is planted
    both = torch.stack([to_dev(vals.astype(dtype)), to_dev(v.astype(dtype))])
    sts = S.check_positive_definite(pat, both)
    assert [s["ok"] for s in sts] == [True, False] and sts[1]["scalar"] == c


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_positive_definite_of_a_jacobian_with_a_zero_column(dtype):
    from baspacho_amd import sparse as S
    m, n, z = 90, 24, 11
    rng = np.random.default_rng(5)
    mask = rng.uniform(size=(m, n)) < 0.2
    mask[np.arange(n), np.arange(n)] = True  # every column is touched
    mask[:, z] |= rng.uniform(size=m) < 0.3
    rows, cols = np.nonzero(mask)
    vals = rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    vals[rows == cols] += 4.0 * np.sign(vals[rows == cols])
    jpat = S.JacobianPattern(rows, cols, m, n)
    full = S.check_positive_definite(jpat, to_dev(vals.astype(dtype)))
    assert full["ok"] and full["scalar"] is None
    vals[cols == z] = 0.0
    v = to_dev(vals.astype(dtype))
    st = S.check_positive_definite(jpat, v)
    print(st)
    assert not st["ok"] and st["scalar"] == z and st["count"] >= 1
    assert st["first"] == int(jpat.solver.scalarPermutation()[z])
    st = S.check_positive_definite(jpat, v, damping=(0.0, 1e-3))
    assert st["ok"] and st["scalar"] is None and st["minDiag"] > 0
    with pytest.raises(ValueError, match="JacobianPattern"):
        S.check_positive_definite(S.SymmetricPattern([0], [0], 1), to_dev(np.ones(1, dtype=dtype)), damping=(0.0, 1.0))
