"""GPU: f(A) v from the Lanczos basis on the MI355X.  bsp_krylov_combine_* must be bitwise
the numpy restatement (matfun_ref.combine) on arbitrary arrays in framed buffers: n = 1, 1023, 1024, 1025, 2049
(one row, the edges of the 1024-row chunk, three chunks), 1 and 3 columns, 1, 7, 8, 9 and 17 terms (the groups of
4 slots the kernel loads together and their tails), 1, 2 and 4 outputs, both precisions, with and without
accumulate, first > 0, slot > 0, per-column limits that differ (0 included) with NaN in every slot and
coefficient at or beyond a column's limit, a batch of 3 against three single calls.  apply_function: the two-pass
route bitwise the kept basis, accuracy against dense eigh at the bounds of the issue (DESIGN.md section 26 lists
them beside the restatement's own errors), identity probes, "inv" against S.solve, the gradient in v, several
functions in one call, the domain errors and call-history independence."""
import ctypes

import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import sparse as S
from buffer_edges import Frame, SENTINEL_BITS
import cg_ref as R
import lanczos_ref as LR
import matfun_ref as MR

SIZES, bs_case = R.BS_SIZES, R.bs_case

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
FOUR = ["inv_sqrt", "sqrt", "inv", "log"]
P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


def _dev(a, tdt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda()


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _dense(n, rows, cols, values):
    A = np.zeros((n, n))
    np.add.at(A, (rows, cols), values)
    return A + np.tril(A, -1).T


# ---- 1. the entry, bitwise against the restatement ----------------------------------------------------------------
_SOLVER = []


def _solver():
    if not _SOLVER:
        idx = np.arange(4)
        _SOLVER.append(S.SymmetricPattern(idx, idx, 4))
    return _SOLVER[0].solver


def _combine_case(sol, rng, n, q, count, nf, dt, accumulate):
    tdt, npdt = DT[dt]
    nb, first, slot = 3, 3, 2
    slots = slot + count + 1
    stride, ostride, ldy = n * q + 3, n * q + 5, count + 2
    nan = np.nan
    # limits: per (member, column), from "nothing" over "part" to "all and more"
    choices = [0, first, first + 1, first + (count + 1) // 2, first + count, first + count + 5]
    limit = np.array([[choices[(2 * m + 3 * c + count) % len(choices)] for c in range(q)] for m in range(nb)], dtype=np.int64)
    limit[0, 0] = (0, first)[count % 2]                                         # at least one column takes no term
    limit[nb - 1, q - 1] = first + count                                        # ... and one takes every term
    basis = np.full((nb, slots, stride), nan)
    basis[:, slot:slot + count, :n * q] = rng.uniform(-1, 1, (nb, count, n * q))
    vs = basis[:, slot:slot + count, :n * q].reshape(nb, count, n, q).astype(npdt)
    y = np.full((nb, q, nf, ldy), nan)
    y[..., :count] = rng.uniform(-2, 2, (nb, q, nf, count))
    for m in range(nb):
        for c in range(q):
            for i in range(count):
                if first + i >= limit[m, c]:                                    # never read: NaN in the slot and in y
                    vs[m, i, :, c] = nan
                    y[m, c, :, i] = nan
    basis[:, slot:slot + count, :n * q] = vs.reshape(nb, count, n * q)
    seed = rng.uniform(-1, 1, (nb, nf, n, q)).astype(npdt)
    bsize, osize = (slots - 1) * stride + n * q, (nf - 1) * ostride + n * q
    fb = Frame([bsize] * nb, npdt)
    fy = Frame([y.size], np.float64)
    fo = Frame([osize] * nb * 2, npdt)          # the outputs of the batched call, then those of the single calls
    for m in range(nb):
        fb.fill(m, basis[m].ravel()[:bsize].astype(npdt))
    fy.fill(0, y.ravel())
    if accumulate:
        for k in range(2 * nb):
            o = fo.host(k)
            for f in range(nf):
                o[f * ostride:f * ostride + n * q] = seed[k % nb, f].ravel()
            fo.fill(k, o)
    fb.seal(), fy.seal(), fo.seal()
    ld = torch.from_numpy(limit).cuda()
    lib = sol._lib
    mid = (I64(stride), I64(slots), I64(slot), I64(count), I64(first))
    torch.cuda.synchronize()
    bp = (ctypes.c_void_p * nb)(*[fb.view(m).data_ptr() for m in range(nb)])
    op = (ctypes.c_void_p * nb)(*[fo.view(m).data_ptr() for m in range(nb)])
    rc = getattr(lib, "bsp_krylov_combine_batched_" + dt)(sol._h, I64(n), I64(q), I32(nf), bp, *mid, P(fy.view(0).data_ptr()),
                                                          I64(ldy), P(ld.data_ptr()), op, I64(ostride), I32(accumulate), I32(nb))
    assert rc == 0, lib.bsp_last_error()
    for m in range(nb):
        rc = getattr(lib, "bsp_krylov_combine_" + dt)(
            sol._h, I64(n), I64(q), I32(nf), P(fb.view(m).data_ptr()), *mid,
            P(fy.view(0).data_ptr() + 8 * m * q * nf * ldy), I64(ldy), P(ld.data_ptr() + 8 * m * q),
            P(fo.view(nb + m).data_ptr()), I64(ostride), I32(accumulate))
        assert rc == 0, lib.bsp_last_error()
    torch.cuda.synchronize()
    what = (n, q, count, nf, dt, accumulate)
    fb.assert_intact(read_only=range(nb), what=what)
    fy.assert_intact(read_only=[0], what=what)
    fo.assert_intact(what=what)
    assert np.array_equal(ld.cpu().numpy(), limit), what
    sent = np.array([SENTINEL_BITS[npdt]], dtype=np.uint64 if npdt is np.float64 else np.uint32).view(npdt)[0]
    for m in range(nb):
        want = MR.combine(vs[m], y[m], limit[m], npdt, out=seed[m] if accumulate else None, first=first)
        assert np.isfinite(want).all(), what
        for k in (m, nb + m):
            o = fo.host(k)
            for f in range(nf):
                got = o[f * ostride:f * ostride + n * q]
                assert got.tobytes() == want[f].tobytes(), (what, "member", m, "single" if k >= nb else "batched", "output", f)
                gap = o[f * ostride + n * q:(f + 1) * ostride]
                assert gap.tobytes() == np.full(len(gap), sent).tobytes(), (what, "the gap behind output", f)
    # the columns with no term: +0 without accumulate, the seed with it (checked above, since want holds them)
    assert (limit <= first).any() and (limit >= first + count).any()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_combine_bitwise_against_the_restatement(n, dt):
    sol = _solver()
    rng = np.random.default_rng(n)
    for q in (1, 3):
        for count in (1, 7, 8, 9, 17):
            for nf in (1, 2, 4):
                for accumulate in (0, 1):
                    _combine_case(sol, rng, n, q, count, nf, dt, accumulate)


def test_combine_three_outputs_and_an_empty_vector():
    sol = _solver()
    _combine_case(sol, np.random.default_rng(3), 1025, 2, 5, 3, "f64", 0)
    _combine_case(sol, np.random.default_rng(3), 1025, 2, 5, 3, "f32", 1)
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    lim = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = sol._lib.bsp_krylov_combine_f64(sol._h, I64(0), I64(1), I32(1), P(one.data_ptr()), I64(0), I64(1), I64(0), I64(1),
                                         I64(0), P(one.data_ptr()), I64(1), P(lim.data_ptr()), P(one.data_ptr()), I64(0), I32(0))
    assert rc == 0, sol._lib.bsp_last_error()


# ---- 2. the two-pass route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_pass_is_bitwise_the_kept_basis(dt):
    tdt, npdt = DT[dt]
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    vd = _dev(values, tdt)
    v0 = np.random.default_rng(31).uniform(-1, 1, (n, 3))
    zd = _dev(v0, tdt)
    kw = dict(steps=24, reorth=None, return_info=True)
    basis, ib = S.apply_function(pat, vd, zd, FOUR, **kw)
    twice, it = S.apply_function(pat, vd, zd, FOUR, memory="two_pass", **kw)
    assert ib["steps"].tolist() == [24] * 3 and it["steps"].tolist() == [24] * 3
    for j in range(4):
        assert basis[j].shape == (n, 3) and bool(torch.isfinite(basis[j]).all())
        assert _bits(basis[j]) == _bits(twice[j]), (dt, FOUR[j])
    for ce in (1, 8):                               # the chunks of the queue change nothing
        again = S.apply_function(pat, vd, zd, FOUR, memory="two_pass", steps=24, reorth=None, check_every=ce)
        assert all(_bits(again[j]) == _bits(basis[j]) for j in range(4)), ce
    # the device route is the restated one
    prod = R.Product(n, rows, cols)
    want, _ = MR.apply_function_model(n, lambda v: prod.mv(values, v, npdt), v0, npdt, FOUR, 24, reorth=None)
    for j in range(4):
        assert _bits(basis[j]) == want[j].tobytes(), (dt, FOUR[j], "restatement")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_pass_beside_a_stopped_and_a_zero_column(dt):
    """the order-255 diagonal that repeats 1, 2, 4 with the ones vector (an invariant subspace after 3 steps) beside a
    zero column and a running column (45 distinct values behind the 255 let a random vector run on)"""
    tdt, npdt = DT[dt]
    d = np.concatenate([np.tile([1.0, 2.0, 4.0], 85), 5.0 + np.arange(45)])
    n = len(d)
    idx = np.arange(n)
    pat = S.SymmetricPattern(idx, idx, n)
    v0 = np.random.default_rng(32).uniform(-1, 1, (n, 3))
    v0[:, 0] = 0.0
    v0[:255, 0] = 1.0
    v0[:, 1] = 0.0
    vd, zd = _dev(d, tdt), _dev(v0, tdt)
    fs = ["inv_sqrt", "log"]
    basis, info = S.apply_function(pat, vd, zd, fs, steps=10, reorth=None, return_info=True)
    twice = S.apply_function(pat, vd, zd, fs, steps=10, reorth=None, memory="two_pass")
    assert info["steps"].tolist() == [3, 0, 10] and info["stop"].tolist() == [LR.INVARIANT, LR.ZERO_START, LR.STEP_LIMIT]
    for j in range(2):
        assert _bits(basis[j]) == _bits(twice[j]), (dt, fs[j])
        zero = basis[j][:, 1].cpu().numpy()
        assert not zero.any() and not np.signbit(zero).any()                 # exactly +0
    want, _ = MR.apply_function_model(n, lambda v: (d[:, None].astype(npdt) * v).astype(npdt), v0, npdt, fs, 10, reorth=None)
    for j in range(2):
        assert _bits(basis[j]) == want[j].tobytes(), (dt, fs[j], "restatement")
    # the stopped column: nothing of the slots beyond its 3 steps leaks in; its result is exact in the subspace
    eps = float(np.finfo(npdt).eps)
    got = basis[0][:, 0].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got[:255], 1 / np.sqrt(d[:255]), rtol=64 * eps)
    assert not got[255:].any()
    assert np.isnan(info["change"][:, 1].cpu().numpy()).all() and bool((info["theta_min"][0] - 1.0).abs() <= 8 * eps)


def test_a_non_finite_column_is_nan():
    d = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    idx = np.arange(5)
    pat = S.SymmetricPattern(idx, idx, 5)
    v0 = np.ones((5, 2))
    v0[1, 0] = np.inf
    for memory, reorth in (("basis", "full"), ("two_pass", None)):
        x, info = S.apply_function(pat, _dev(d, torch.float64), _dev(v0, torch.float64), "inv", steps=5, reorth=reorth,
                                   memory=memory, return_info=True)
        assert info["stop"].tolist() == [LR.NON_FINITE, LR.INVARIANT] or info["stop"].tolist() == [LR.NON_FINITE, LR.STEP_LIMIT]
        assert bool(torch.isnan(x[:, 0]).all())
        np.testing.assert_allclose(x[:, 1].cpu().numpy(), 1 / d, rtol=1e-13)


# ---- 3. accuracy against dense eigh ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,bound", [("f64", 1e-11), ("f32", 1e-3)])
def test_accuracy_at_n_steps_with_full_reorthogonalisation(dt, bound):
    tdt, npdt = DT[dt]
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    v0 = np.random.default_rng(21).uniform(-1, 1, (n, 2)).astype(npdt)
    Ad = _dense(n, rows, cols, values.astype(npdt).astype(np.float64))
    vd, zd = _dev(values, tdt), _dev(v0, tdt)
    outs, info = S.apply_function(pat, vd, zd, FOUR, steps=n, return_info=True)
    assert info["steps"].tolist() == [n, n] and info["change"].shape == (4, 2)
    for j, f in enumerate(FOUR):
        err = MR.rel_err(outs[j].cpu().numpy(), MR.dense_function(Ad, f, v0))
        print("bs_case, %d steps, full, %s, %s: relative error %s (bound %g)" % (n, dt, f, err, bound))
        assert (err <= bound).all(), (f, err)
    if dt == "f64":
        x = S.apply_function(pat, vd, zd, ("exp", 0.5), steps=24)
        err = MR.rel_err(x.cpu().numpy(), MR.dense_function(Ad, ("exp", 0.5), v0))
        print("bs_case, 24 steps, full, f64, exp(-A / 2): relative error %s (bound 1e-12)" % err)
        assert (err <= 1e-12).all(), err
        # steps is capped at n; a single vector [n] comes back as [n]
        x1 = S.apply_function(pat, vd, zd[:, 0].contiguous(), "log", steps=500)
        assert x1.shape == (n,) and _bits(x1) == _bits(outs[3][:, 0])


@pytest.mark.parametrize("dt,bound", [("f64", 1e-12), ("f32", 1e-5)])
def test_accuracy_of_the_plain_recurrence_in_both_memory_modes(dt, bound):
    tdt, npdt = DT[dt]
    n = 1500
    rows, cols, values = R.tridiagonal(n)
    pat = S.SymmetricPattern(rows, cols, n)
    v0 = np.random.default_rng(22).uniform(-1, 1, (n, 2)).astype(npdt)
    Ad = _dense(n, rows, cols, values.astype(npdt).astype(np.float64))
    want = [MR.dense_function(Ad, f, v0) for f in FOUR]
    for memory in ("basis", "two_pass"):
        outs = S.apply_function(pat, _dev(values, tdt), _dev(v0, tdt), FOUR, steps=48, reorth=None, memory=memory)
        for j, f in enumerate(FOUR):
            err = MR.rel_err(outs[j].cpu().numpy(), want[j])
            print("tridiagonal(1500), 48 steps, reorth None, %s, %s, %s: relative error %s (bound %g)" % (memory, dt, f, err, bound))
            assert (err <= bound).all(), (memory, f, err)


# ---- 4. identity probes, 5. inv against solve ---------------------------------------------------------------------
def test_identity_probes_and_sample_lanczos():
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    vd = _dev(values, torch.float64)
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    Xd = S.apply_function(pat, vd, eye, "inv_sqrt", steps=n)
    X = Xd.cpu().numpy()
    inv = np.linalg.inv(A)
    e1 = np.abs(X @ X.T - inv).max() / np.abs(inv).max()
    e2 = np.abs(X - X.T).max() / np.abs(X).max()
    print("identity probes: max |X X^T - inv(A)| / max |inv(A)| = %g, max |X - X^T| / max |X| = %g (bounds 1e-11)" % (e1, e2))
    assert e1 <= 1e-11 and e2 <= 1e-11
    mu = _dev(np.random.default_rng(41).uniform(-1, 1, (n, n)), torch.float64)
    x = S.sample_lanczos(pat, vd, eye, mu, steps=n)
    assert _bits(x) == _bits(mu + Xd)
    assert _bits(S.sample_lanczos(pat, vd, eye, steps=n)) == _bits(Xd)
    C = S.sample_cov_lanczos(pat, vd, eye, steps=n).cpu().numpy()
    assert np.abs(C @ C - A).max() <= 1e-11 * np.abs(A).max()
    with pytest.raises(ValueError, match="mu must be a tensor of the result's shape"):
        S.sample_lanczos(pat, vd, eye, mu[0], steps=n)


def test_inv_at_n_steps_against_solve():
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    vd = _dev(values, torch.float64)
    b = _dev(np.random.default_rng(51).uniform(-1, 1, (n, 3)), torch.float64)
    x = S.apply_function(pat, vd, b, "inv", steps=n)
    want = S.solve(pat, vd, b)
    err = (torch.linalg.norm(x - want, dim=0) / torch.linalg.norm(want, dim=0)).cpu().numpy()
    print("inv at n steps against S.solve: relative error", err, "(bound 1e-10)")
    assert (err <= 1e-10).all()
    # a batch, and vectors shared by its members: member 0 is the single call
    vb = torch.stack([vd, 2 * vd])
    xs = S.apply_function(pat, vb, b, "inv", steps=n)
    xb = S.apply_function(pat, vb, torch.stack([b, b]), "inv", steps=n)
    assert xs.shape == (2, n, 3) and _bits(xs) == _bits(xb) and _bits(xs[0]) == _bits(x)
    assert float((2 * xs[1] - x).abs().max()) <= 1e-10 * float(x.abs().max())


# ---- 6. the gradient in v --------------------------------------------------------------------------------------
def test_gradient_in_v():
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    vd = _dev(values, torch.float64)
    rng = np.random.default_rng(61)
    v0, g, g2 = rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2))
    v = _dev(v0, torch.float64).requires_grad_(True)
    x = S.apply_function(pat, vd, v, "inv_sqrt", steps=n)
    x.backward(_dev(g, torch.float64))
    err = MR.rel_err(v.grad.cpu().numpy(), MR.dense_function(A, "inv_sqrt", g))
    print("gradient in v, inv_sqrt: relative error", err, "(bound 1e-10)")
    assert (err <= 1e-10).all()
    # two functions: the gradients add; the mean of sample_lanczos gets the identity
    v = _dev(v0, torch.float64).requires_grad_(True)
    mu = torch.zeros(n, 2, dtype=torch.float64, device="cuda", requires_grad=True)
    a, b = S.apply_function(pat, vd, v, ["log", ("exp", 0.5)], steps=n)
    (a * _dev(g, torch.float64)).sum().backward(retain_graph=True)
    (b * _dev(g2, torch.float64)).sum().backward()
    want = MR.dense_function(A, "log", g) + MR.dense_function(A, ("exp", 0.5), g2)
    assert (MR.rel_err(v.grad.cpu().numpy(), want) <= 1e-10).all()
    z = _dev(v0, torch.float64).requires_grad_(True)
    S.sample_lanczos(pat, vd, z, mu, steps=n).backward(_dev(g, torch.float64))
    assert _bits(mu.grad) == _bits(_dev(g, torch.float64))
    assert (MR.rel_err(z.grad.cpu().numpy(), MR.dense_function(A, "inv_sqrt", g)) <= 1e-10).all()
    with pytest.raises(ValueError, match="gradients in values .* are not provided"):
        S.apply_function(pat, vd.clone().requires_grad_(True), v, "inv")


# ---- 7. several functions, 8. the domain, 9. history ---------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_several_functions_are_bitwise_the_single_calls(dt):
    tdt, npdt = DT[dt]
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    vd = _dev(values, tdt)
    zd = _dev(np.random.default_rng(71).uniform(-1, 1, (n, 3)), tdt)
    fs = ["inv_sqrt", ("exp", 0.25), ("pow", 2), "log"]
    for kw in (dict(steps=20), dict(steps=20, reorth=None, memory="two_pass")):
        outs = S.apply_function(pat, vd, zd, fs, **kw)
        assert isinstance(outs, tuple) and len(outs) == 4
        for j, f in enumerate(fs):
            assert _bits(S.apply_function(pat, vd, zd, f, **kw)) == _bits(outs[j]), (dt, f, kw)
        pair = S.apply_function(pat, vd, zd, fs[1:3], **kw)
        assert _bits(pair[0]) == _bits(outs[1]) and _bits(pair[1]) == _bits(outs[2])
    with pytest.raises(ValueError, match="sequence of 1 .. 4"):
        S.apply_function(pat, vd, zd, fs + ["inv"])


def test_domain_errors_and_a_callable():
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    v = values.copy()
    v[rows == cols] -= np.linalg.eigvalsh(A)[1] * 1.5          # shifts the lowest eigenvalue below zero
    z = _dev(np.random.default_rng(81).uniform(-1, 1, (n, 2)), torch.float64)
    with pytest.raises(B.FactorizationError, match=r"Ritz value -\S+ of column 0 is <= 0, outside the domain of inv_sqrt") as e:
        S.apply_function(pat, _dev(v, torch.float64), z, "inv_sqrt", steps=n)
    assert e.value.status["column"] == 0 and e.value.status["theta_min"] < 0
    with pytest.raises(B.FactorizationError, match="column 0 of batch member 1"):
        S.apply_function(pat, _dev(np.stack([values, v]), torch.float64), z, "log", steps=n)
    # the identity as a callable returns A v, on the indefinite matrix too
    for vals in (values, v):
        got = S.apply_function(pat, _dev(vals, torch.float64), z, lambda t: t, steps=n).cpu().numpy()
        want = _dense(n, rows, cols, vals) @ z.cpu().numpy()
        err = MR.rel_err(got, want)
        print("callable t -> t against A v: relative error", err, "(bound 1e-13)")
        assert (err <= 1e-13).all()
    with pytest.raises(ValueError, match="finite array"):
        S.apply_function(pat, _dev(values, torch.float64), z, lambda t: np.log(t - 1e6), steps=8)


def test_refusals():
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    v, z = _dev(values, torch.float64), _dev(np.ones((n, 2)), torch.float64)
    with pytest.raises(ValueError, match="needs reorth=None"):
        S.apply_function(pat, v, z, "inv", memory="two_pass")
    with pytest.raises(ValueError, match="memory must be"):
        S.apply_function(pat, v, z, "inv", memory="ring")
    with pytest.raises(ValueError, match="f must be"):
        S.apply_function(pat, v, z, "cos")
    with pytest.raises(ValueError, match="steps"):
        S.apply_function(pat, v, z, "inv", steps=0)
    with pytest.raises(TypeError, match="dtype"):
        S.apply_function(pat, v, z.float(), "inv")
    with pytest.raises(ValueError, match=r"\[B, n, q\] or a shared"):
        S.apply_function(pat, torch.stack([v, v]), torch.ones(2, n + 1, dtype=torch.float64, device="cuda"), "inv")


def test_history_independence():
    rows, cols, values, A, n = bs_case()
    vd = _dev(values, torch.float64)
    zd = _dev(np.random.default_rng(91).uniform(-1, 1, (n, 3)), torch.float64)
    fresh = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    used = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    S.solve(used, vd, zd)                                        # factored and solved
    S.solve_cg(used, vd, zd, precond="jacobi", max_steps=5)      # ... and run CG
    S.logdet_slq(used, vd, probes=2, steps=4)
    for kw in (dict(steps=24), dict(steps=24, reorth=None, memory="two_pass")):
        a = S.apply_function(fresh, vd, zd, ["inv_sqrt", "log"], **kw)
        b = S.apply_function(used, vd, zd, ["inv_sqrt", "log"], **kw)
        assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]), kw
