"""The buffer-edge contract holds for the references, and the checks of tests/buffer_edges.py can fail
(no GPU needed).

1. The CPU oracle (oracle/cref.py) factors and solves bitwise the same with the sentinel NaN in every
   strictly-upper diagonal-block element, with ld = n + 5 and sentinel padding rows, which it leaves alone.
2. The numpy restatements (the factor's and the partial factor's adjoint recurrences, the references of
   selected inversion, pattern_grad_ref) are bitwise unchanged by the sentinel in the upper input elements.
3. Simulated mistakes: a factor that takes one diagonal-block element from the upper triangle, a solve that
   indexes its columns with n in place of ld, a store one word past / before a payload, a store to a
   read-only payload.  Each must fail its check; the correct twin must pass."""
import numpy as np
import pytest

import chol_adjoint_ref
import partial_adjoint_ref
from autograd_ref import element_coords, pattern_grad_ref
from buffer_edges import (GUARD, SENTINEL, SENTINEL_BITS, Frame, assert_padding_intact, bitwise_equal, clear_upper,
                          framed, is_sentinel, poison_upper, strided, unpack, upper_words)
from helpers import solver_random
from kf_structures import bipartite, random_with_range
from known_factor import known_factor_data, sparsify
from oracle import cref
from selinv_cases import build_case
from selinv_ref import dense_reference, oracle_columns
from stress_cases import width_solver

DTYPES = [np.float64, np.float32]
LAZY = {"lazy_plan": 1}

STRUCTURES = {
    "random_with_range": lambda: random_with_range(7, LAZY),
    "bipartite": lambda: bipartite(200, 9, 3, 6, seed=8, hip_options=LAZY),
    "merged": lambda: solver_random(58, fill=0.03, elim=(0, 60), ranges=[0, 60], model="hip", psize_seed=48)[0],
    "width65_tail70": lambda: width_solver(65, 70, LAZY),
}
_sols = {}


def _sol(name):
    if name not in _sols:
        _sols[name] = STRUCTURES[name]()
    return _sols[name]


def _rhs(n, nrhs, dtype, seed):
    return np.random.default_rng(seed).standard_normal((n, nrhs)).astype(dtype).astype(np.float64)


# ---- the helper itself --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(STRUCTURES))
def test_upper_words_are_the_elements_above_the_diagonal(name):
    sol = _sol(name)
    up = upper_words(sol)  # (asserts ~lowerMask() == (i < j))
    i, j = element_coords(sol)
    assert len(up) > 0 and (i[up] < j[up]).all() and len(up) == int((i < j).sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_sentinel_is_a_quiet_nan_that_survives_copies(dtype):
    import torch
    s = SENTINEL[dtype]
    assert np.isnan(s) and s.dtype == np.dtype(dtype)
    a = np.arange(7, dtype=dtype)
    a[3] = s
    assert is_sentinel(a).tolist() == [False] * 3 + [True] + [False] * 3
    fr = Frame([7, 4], dtype, device="cpu")
    fr.fill(0, a)
    assert bitwise_equal(fr.host(0), a)
    assert is_sentinel(fr.host(1)).all() and is_sentinel(fr.base.numpy()).sum() == fr.total - 6
    t = torch.from_numpy(a.copy())
    assert bitwise_equal(t.clone().numpy(), a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frame_layout(dtype):
    fr = Frame([10, 7, 1, 64], dtype, device="cpu")
    assert fr.offsets[0] == GUARD + 1
    end = 0
    for k, (o, s) in enumerate(zip(fr.offsets, fr.sizes)):
        assert o % 2 == 1 and o - end >= GUARD, (k, o, end)
        assert (o * np.dtype(dtype).itemsize) % 16 != 0
        v = fr.view(k)
        assert v.is_contiguous() and v.numel() == s and v.data_ptr() == fr.base.data_ptr() + o * v.element_size()
        end = o + s
    assert fr.total - end == GUARD
    fr.seal().assert_intact(read_only=range(4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_round_trip_and_poison(dtype):
    import torch
    b = _rhs(11, 3, dtype, 1)
    v = strided(b, 16, dtype)
    assert v.dtype == np.dtype(dtype) and v.size == 48
    assert np.array_equal(unpack(v, 11, 16, 3), b)
    assert is_sentinel(v).sum() == 15
    assert_padding_intact(v, 11, 16, 3)
    sol = _sol("width65_tail70")
    a = np.random.default_rng(2).standard_normal(sol.dataSize()).astype(dtype)
    host = poison_upper(a.copy(), sol)
    dev = poison_upper(torch.from_numpy(a.copy()), sol).numpy()
    assert bitwise_equal(host, dev)
    up = upper_words(sol)
    assert is_sentinel(host)[up].all() and is_sentinel(host).sum() == len(up)
    mask = sol.lowerMask()
    assert bitwise_equal(host[mask], a[mask])
    assert not np.isnan(clear_upper(host, sol)).any()


# ---- 1. the oracle under poison -------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(STRUCTURES))
def test_oracle_ignores_upper_elements_and_padding(name, dtype):
    sol = _sol(name)
    sk, ranges = cref.SkelHandle(sol.skel()), sol.sparseEliminationRanges()
    n, nrhs, ld = sol.order(), 3, sol.order() + 5
    mask = sol.lowerMask()
    kf = known_factor_data(sol, 3, dtype)
    clean = cref.factor(sk, kf.data.copy(), ranges)
    pois = cref.factor(sk, poison_upper(kf.data.copy(), sol), ranges)
    assert not np.isnan(clean[mask]).any()
    assert bitwise_equal(clean[mask], pois[mask]), "the oracle's factor read an upper element"
    kf.check_factor(pois, "oracle under poison")
    L = poison_upper(pois.copy(), sol)
    b = _rhs(n, nrhs, dtype, 4)
    for fn in (cref.solve, cref.solve_l, cref.solve_lt):
        want = fn(sk, clean, b.T.ravel().astype(dtype), n, nrhs)
        got = fn(sk, L, strided(b, ld, dtype), ld, nrhs)
        assert_padding_intact(got, n, ld, nrhs, fn.__name__)
        assert bitwise_equal(got.reshape(nrhs, ld)[:, :n], want.reshape(nrhs, n)), fn.__name__
    assert bitwise_equal(L[mask], pois[mask]) and is_sentinel(L)[~mask].all()


# ---- 2. the numpy restatements under poison -----------------------------------------------------

ADJOINT_STRUCTURES = {"mixed_owners": lambda: build_case("mixed_owners")[0],
                      "random_elim": lambda: solver_random(3, fill=0.037, elim=(0, 60))[0]}


@pytest.mark.parametrize("name", list(ADJOINT_STRUCTURES))
def test_adjoint_recurrences_ignore_upper_elements(name):
    sol = ADJOINT_STRUCTURES[name]()
    kf = known_factor_data(sol, 5, np.float64, rho=0.5)
    L = chol_adjoint_ref.dense_factor(sol, kf.data)
    lbar = chol_adjoint_ref.lbar_random(sol, 11)
    plan = sol._testSelInvPlan()
    want = chol_adjoint_ref.recurrence_np(sol, L, lbar, plan)
    got = chol_adjoint_ref.recurrence_np(sol, poison_upper(L.copy(), sol), poison_upper(lbar.copy(), sol), plan)
    assert not np.isnan(want).any() and bitwise_equal(got, want)
    sp = partial_adjoint_ref.splits(sol)
    span = sp[len(sp) // 2]
    assert 0 < span < sol.numSpans()
    P = cref.factor(sol.skel(), kf.data.copy(), sol.sparseEliminationRanges(), 0, span)
    want = partial_adjoint_ref.recurrence_np(sol, P, lbar, span)
    got = partial_adjoint_ref.recurrence_np(sol, poison_upper(P.copy(), sol), poison_upper(lbar.copy(), sol), span)
    assert not np.isnan(want).any() and bitwise_equal(got, want)


@pytest.mark.parametrize("name", list(ADJOINT_STRUCTURES))
def test_selected_inversion_references_ignore_upper_elements(name):
    sol = ADJOINT_STRUCTURES[name]()
    kf = known_factor_data(sol, 6, np.float64, rho=0.5)
    pois = poison_upper(kf.data.copy(), sol)
    for a, b in zip(dense_reference(sol, kf.data), dense_reference(sol, pois)):
        assert bitwise_equal(np.asarray(a), np.asarray(b))
    spans = [0, sol.numSpans() // 2, sol.numSpans() - 1]
    (ia, Xa), (ib, Xb) = oracle_columns(sol, kf.data, spans), oracle_columns(sol, pois, spans)
    assert np.array_equal(ia, ib) and not np.isnan(Xa).any() and bitwise_equal(Xa, Xb)


def test_pattern_grad_ref_ignores_upper_elements():
    sol = _sol("random_with_range")
    rng = np.random.default_rng(8)
    n, k = sol.order(), 5
    Z = rng.uniform(-1, 1, sol.dataSize())
    U, V = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    for kw in (dict(Z=Z, s=0.75), dict(U=U, V=V, alpha=-1.5), dict(Z=Z, s=0.75, U=U, V=V, alpha=-1.5)):
        want = pattern_grad_ref(sol, **kw)
        if "Z" in kw:
            kw = dict(kw, Z=poison_upper(Z.copy(), sol))
        got = pattern_grad_ref(sol, **kw)
        assert not np.isnan(want).any() and bitwise_equal(got, want)


# ---- 3. the checks catch mistakes ---------------------------------------------------------------

def _column_cholesky(D, swap=None):
    """Cholesky by columns of the matrix whose element (i, j), i >= j, is read from D[i, j]; swap=(i, j):
    that one element is read from D[j, i] instead (the mistake)"""
    A = np.tril(D).copy()
    if swap is not None:
        A[swap] = D[swap[1], swap[0]]
    n = len(A)
    L = np.zeros((n, n))
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = c / np.sqrt(c[0])
    return L


@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_reading_one_upper_element_fails(dtype):
    sol = _sol("width65_tail70")
    kf = known_factor_data(sol, 11, dtype)
    D = sol.densify(poison_upper(kf.data.copy(), sol).astype(np.float64))
    assert np.isnan(D[0, 1]) and np.isnan(D[65, 66]) and not np.isnan(np.tril(D)).any()
    good = sparsify(sol, _column_cholesky(D), dtype)
    kf.check_factor(good, "correct simulated factor")
    for swap in ((1, 0), (64, 3), (66, 65), (134, 133)):  # (inside the two lumps' diagonal blocks)
        bad = sparsify(sol, _column_cholesky(D, swap), dtype)
        assert np.isnan(bad[sol.lowerMask()]).any(), swap
        with pytest.raises(AssertionError, match="known-factor check failed"):
            kf.check_factor(bad, ("upper element read", swap))


@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_indexing_columns_with_n_fails(dtype):
    sol = _sol("width65_tail70")
    kf = known_factor_data(sol, 12, dtype)
    n, nrhs, ld = sol.order(), 3, sol.order() + 5
    b = _rhs(n, nrhs, dtype, 3)
    x = np.linalg.solve(kf.A, b)
    good = strided(x, ld, dtype)
    assert_padding_intact(good, n, ld, nrhs)
    kf.check_solve(b, unpack(good, n, ld, nrhs))
    bad = strided(b, ld, dtype)
    for c in range(nrhs):  # (column c written at c * n)
        bad[c * n:c * n + n] = x[:, c].astype(dtype)
    with pytest.raises(AssertionError, match="padding row"):
        assert_padding_intact(bad, n, ld, nrhs)
    with pytest.raises(AssertionError, match="known-factor check failed"):
        kf.check_solve(b, unpack(bad, n, ld, nrhs))
    # one row too many in one column only
    bad = good.copy()
    bad[2 * ld + n] = 0.0
    with pytest.raises(AssertionError, match="row %d of column 2" % n):
        assert_padding_intact(bad, n, ld, nrhs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stray_stores_fail(dtype):
    a = [np.arange(33, dtype=dtype), np.arange(8, dtype=dtype), np.arange(5, dtype=dtype)]

    def fresh():
        return framed(dtype, a, device="cpu")

    fr = fresh()
    fr.assert_intact(read_only=(0, 1, 2))
    fr.view(1)[3] = 7.0  # an operand that may be written
    fr.assert_intact(read_only=(0, 2))
    for k in range(3):
        o, s = fr.offsets[k], fr.sizes[k]
        for at, where in ((o + s, "past"), (o - 1, "before"), (o + s + GUARD - 1, "far past"), (o - GUARD, "far before")):
            fr = fresh()
            fr.base[at] = 1.0
            with pytest.raises(AssertionError, match="outside the payloads"):
                fr.assert_intact(what=(k, where))
        fr = fresh()
        fr.view(k)[s - 1] = -1.0
        fr.assert_intact(read_only=[q for q in range(3) if q != k])
        with pytest.raises(AssertionError, match="read-only operand"):
            fr.assert_intact(read_only=(k,))
    # a store of another NaN, and of the sentinel of the other width, is seen as well
    fr = fresh()
    fr.base[fr.offsets[0] - 1] = float("nan")
    with pytest.raises(AssertionError, match="outside the payloads"):
        fr.assert_intact()
    # a read-only payload rewritten with a NaN of another payload (equal as floats, not as words)
    b = [np.full(4, SENTINEL[dtype])]
    fr = framed(dtype, b, device="cpu")
    fr.view(0)[2] = float("nan")
    assert SENTINEL_BITS[dtype] != int(np.array([np.nan], dtype=dtype).view(np.uint64 if dtype == np.float64 else np.uint32)[0])
    with pytest.raises(AssertionError, match="read-only operand"):
        fr.assert_intact(read_only=(0,))
