"""GPU: the device-resident conjugate gradient on the MI355X.  sparse.solve_cg must be
bitwise the numpy restatement (cg_ref.py) -- x, the state records and the preconditioner's status -- for
precond None, "jacobi" and "block_jacobi", in f64 and f32, at the sizes that cross every boundary of the
reductions (n = 1, 255, 256, 1024, 1025, 2049, and 256 * 1024 + 1 for a second pass over more than 256
partials), with 1 and 3 right-hand sides and batches of 1 and 3.  Within the GPU results: the same bits for
every check_every, for a column alone and beside others, for a matrix alone and in a batch, for a fresh
pattern and a used one; a stopped column frozen while its neighbour runs on.  "factor32" and DevicePCG over
TrailingOperator are checked by their true residual and their step count; gradients against S.solve's."""
import functools

import numpy as np
import pytest
import torch

from baspacho_amd import cg as CG
from baspacho_amd import pcg
from baspacho_amd import sparse as S
from assembly_ref import dense_user
import cg_ref as R

SIZES, TOL, bs_case = R.BS_SIZES, R.TOL, R.bs_case

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64, 1e-8), "f32": (torch.float32, np.float32, 1e-4)}
NS = [1, 255, 256, 1024, 1025, 2049]
CYCLE = [1, 3, 9, 32, 2]  # param sizes, repeated and cut to n


def _dev(a, tdt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda()


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _sizes(n):
    out = []
    while sum(out) < n:
        out.append(min(CYCLE[len(out) % len(CYCLE)], n - sum(out)))
    return out


@functools.lru_cache(maxsize=None)
def _tri_case(n):
    """a tridiagonal matrix with a varied diagonal, every 7th diagonal entry given twice, three sets of values;
    b [3, n, 3] with one zero column"""
    rng = np.random.default_rng(n)
    rows, cols, _ = R.tridiagonal(n)
    dup = np.arange(0, n, 7)
    rows, cols = np.concatenate([rows, dup]), np.concatenate([cols, dup])
    values = np.stack([np.concatenate([3.0 + rng.uniform(0, 1, n), -1.0 + rng.uniform(-0.1, 0.1, n - 1),
                                       rng.uniform(0.2, 0.6, len(dup))]) for _ in range(3)])
    b = rng.uniform(-1, 1, (3, n, 3))
    b[1, :, 2] = 0.0
    sizes = _sizes(n)
    return rows, cols, values, b, sizes, S.SymmetricPattern(rows, cols, n, param_sizes=sizes)


def _check_against_model(got_x, info, want_x, st, status, j_of, what):
    assert _bits(got_x) == _bits(want_x), (what, "x")
    state = info["state"].cpu().numpy().reshape(-1, 12)
    for j in range(state.shape[0]):
        np.testing.assert_array_equal(state[j], R.record_words(st, j_of(j)), err_msg="%s column %d" % (what, j))
    if status is not None:
        np.testing.assert_array_equal(info["precond_status"].cpu().numpy(), status, err_msg=what)


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", NS)
def test_bitwise_against_the_restatement(n, dt, precond):
    tdt, npdt, tol = DT[dt]
    rows, cols, values, b, sizes, pat = _tri_case(n)
    kw = dict(precond=precond, tol=tol, max_steps=40)
    vd, bd = _dev(values, tdt), _dev(b, tdt)
    xb, ib = S.solve_cg(pat, vd, bd, return_info=True, **kw)           # batch of 3, q = 3
    x1, i1 = S.solve_cg(pat, vd[0], bd[0, :, 0].contiguous(), return_info=True, **kw)  # one matrix, one vector
    torch.cuda.synchronize()
    stops = set()
    for m in range(3):
        want, st, status = R.entries_model(n, rows, cols, values[m], b[m], npdt, precond, param_sizes=sizes, tol=tol,
                                           max_steps=40)
        sub = {"state": ib["state"][m]}
        if precond is not None:
            sub["precond_status"] = ib["precond_status"][m]
        _check_against_model(xb[m], sub, want, st, status, lambda j: j, (n, dt, precond, m))
        np.testing.assert_array_equal(ib["iterations"][m].cpu().numpy(), st["iterations"])
        np.testing.assert_array_equal(ib["stop"][m].cpu().numpy(), st["stop"])
        stops |= set(st["stop"].tolist())
        if m == 0:  # the single call, q = 1: bitwise column 0 of member 0
            assert x1.shape == (n,) and _bits(x1) == _bits(want[:, 0])
            np.testing.assert_array_equal(i1["state"].cpu().numpy(), R.record_words(st, 0))
            assert i1["iterations"].shape == () and i1["relres"].shape == ()
    assert R.ZERO_RHS in stops and R.CONVERGED in stops and R.RUNNING not in stops
    rel = ib["relres"].cpu().numpy()
    assert rel.shape == (3, 3) and rel[1, 2] == 0.0 and not xb[1, :, 2].any()


def test_second_pass_over_more_than_256_partials():
    n = 256 * 1024 + 1
    rows, cols, values = R.tridiagonal(n, 2.5, -1.0)
    rng = np.random.default_rng(9)
    values = values + np.concatenate([rng.uniform(0, 1, n), np.zeros(n - 1)])
    b = rng.uniform(-1, 1, n)
    pat = S.SymmetricPattern(rows, cols, n)
    x, info = S.solve_cg(pat, _dev(values, torch.float64), _dev(b, torch.float64), precond=None, tol=1e-12, max_steps=3,
                         check_every=None, return_info=True)
    want, st, _ = R.entries_model(n, rows, cols, values, b, np.float64, None, tol=1e-12, max_steps=3)
    assert _bits(x) == _bits(want)
    np.testing.assert_array_equal(info["state"].cpu().numpy(), R.record_words(st, 0))
    assert int(info["stop"]) == R.STEP_LIMIT and int(info["iterations"]) == 3


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_same_bits_for_every_check_every_column_and_batch(dt, precond):
    tdt, npdt, tol = DT[dt]
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    rng = np.random.default_rng(11)
    vals = np.stack([values, values * rng.uniform(0.999, 1.001, len(values))])
    b = rng.uniform(-1, 1, (2, n, 3))
    b[0, :, 1] = np.linalg.eigh(A)[1][:, 0]       # an eigenvector: plain CG stops after a step or two
    b[1, :, 2] = 0.0                               # and a zero column, which never starts
    vd, bd = _dev(vals, tdt), _dev(b, tdt)
    kw = dict(precond=precond, tol=tol, max_steps=60, return_info=True)
    ref_x, ref_i = S.solve_cg(pat, vd, bd, check_every=8, **kw)
    its = ref_i["iterations"].cpu().numpy()
    assert its.min() < its.max()
    for ce in (1, None):
        x, i = S.solve_cg(pat, vd, bd, check_every=ce, **kw)
        assert _bits(x) == _bits(ref_x) and _bits(i["state"]) == _bits(ref_i["state"]), ce
    for m in range(2):                             # a matrix alone
        x, i = S.solve_cg(pat, vd[m], bd[m], **kw)
        assert _bits(x) == _bits(ref_x[m]) and _bits(i["state"]) == _bits(ref_i["state"][m])
        for j in range(3):                         # a column alone
            x, i = S.solve_cg(pat, vd[m], bd[m, :, j].contiguous(), **kw)
            assert _bits(x) == _bits(ref_x[m, :, j]) and _bits(i["state"]) == _bits(ref_i["state"][m, j])
    # a pattern that has already run other operations
    used = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    S.solve(used, vd.double(), bd.double())
    S.matvec(used, vd, bd)
    S.solve_cg(used, vd[0], bd[0], precond="jacobi", max_steps=2)
    x, i = S.solve_cg(used, vd, bd, check_every=8, **kw)
    assert _bits(x) == _bits(ref_x) and _bits(i["state"]) == _bits(ref_i["state"])


def test_frozen_column():
    """the eigenvector column's x is bitwise what it was at its stop while its neighbour runs 20 more steps"""
    n = 64
    rows, cols, values = R.tridiagonal(n)
    k = np.arange(1, n + 1)
    b = np.stack([np.sin(np.pi * 3 * k / (n + 1)), np.random.default_rng(0).uniform(-1, 1, n)], axis=1)
    pat = S.SymmetricPattern(rows, cols, n)
    vd, bd = _dev(values, torch.float64), _dev(b, torch.float64)
    x1, i1 = S.solve_cg(pat, vd, bd, precond=None, tol=1e-12, max_steps=1, return_info=True)
    x21, i21 = S.solve_cg(pat, vd, bd, precond=None, tol=1e-12, max_steps=21, check_every=None, return_info=True)
    assert i1["stop"].tolist() == [R.CONVERGED, R.STEP_LIMIT] and i1["iterations"].tolist() == [1, 1]
    assert i21["stop"].tolist() == [R.CONVERGED, R.STEP_LIMIT] and i21["iterations"].tolist() == [1, 21]
    assert _bits(x21[:, 0]) == _bits(x1[:, 0])
    assert _bits(i21["state"][0, :9]) == _bits(i1["state"][0, :9])  # (word 9 is the step limit, 21 against 1)
    assert _bits(x21[:, 1]) != _bits(x1[:, 1])
    x0, _, _ = R.entries_model(n, rows, cols, values, b, np.float64, None, tol=1e-12, max_steps=21)
    assert _bits(x21) == _bits(x0)


@pytest.mark.parametrize("case", ["breakdown", "nan", "bad_block"])
def test_stops_and_status_on_the_device(case):
    if case == "breakdown":
        pat = S.SymmetricPattern([0, 1], [0, 1], 2)
        x, i = S.solve_cg(pat, _dev([1.0, -1.0], torch.float64), _dev([1.0, 1.0], torch.float64), precond=None,
                          return_info=True)
        assert int(i["stop"]) == R.BREAKDOWN and int(i["iterations"]) == 0 and x.tolist() == [0.0, 0.0]
        assert CG.read_state(i["state"])["stopReason"] == "breakdown"
        x, i = S.solve_cg(pat, _dev([1.0, -1.0], torch.float64), _dev([1.0, 1.0], torch.float64), precond="jacobi",
                          return_info=True)
        assert i["precond_status"].tolist() == [1, 1] and bool(torch.isfinite(x).all())
        return
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    b = np.ones((n, 2))
    v = values.copy()
    if case == "nan":
        v[3] = np.nan
        x, i = S.solve_cg(pat, _dev(v, torch.float64), _dev(b, torch.float64), precond=None, return_info=True)
        assert i["stop"].tolist() == [R.NON_FINITE] * 2 and i["iterations"].tolist() == [0, 0]
        return
    bs = np.concatenate([[0], np.cumsum(SIZES)])
    scalar = int(bs[2] + 4)
    v[int(np.nonzero((rows == scalar) & (cols == scalar))[0][0])] = -5.0
    for precond in ("jacobi", "block_jacobi"):
        x, i = S.solve_cg(pat, _dev(v, torch.float64), _dev(b, torch.float64), precond=precond, max_steps=5,
                          return_info=True)
        _, _, status = R.entries_model(n, rows, cols, v, b, np.float64, precond, param_sizes=SIZES, max_steps=5)
        got = i["precond_status"].tolist()
        assert got == status.tolist() and got[1] == 1 and bs[2] <= got[0] <= scalar
        assert bool(torch.isfinite(x).all())
        if precond == "jacobi":
            assert got == [scalar, 1]


def _f32_cholesky_precond(M):
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(M.astype(np.float32))
    return lambda r: solve_triangular(L.T, solve_triangular(L, r.astype(np.float32), lower=True),
                                      lower=False).astype(np.float64)


def test_factor32_converges_to_the_true_residual():
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    b = np.random.default_rng(2).uniform(-1, 1, (n, 3))
    x, i = S.solve_cg(pat, _dev(values, torch.float64), _dev(b, torch.float64), precond="factor32", tol=TOL,
                      return_info=True)
    assert i["stop"].tolist() == [R.CONVERGED] * 3 and "precond_status" not in i
    xh = x.cpu().numpy()
    true_res = np.linalg.norm(b - A @ xh, axis=0) / np.linalg.norm(b, axis=0)
    print("factor32: iterations", i["iterations"].tolist(), "true residual", true_res)
    assert (true_res <= 2 * TOL).all(), true_res
    _, st = R.cg_model(n, lambda p: A @ p, b, np.float64, _f32_cholesky_precond(A), tol=TOL, max_steps=100)
    assert (i["iterations"].cpu().numpy() <= st["iterations"] + 1).all(), (i["iterations"], st["iterations"])
    with pytest.raises(TypeError, match="float64"):
        S.solve_cg(pat, _dev(values, torch.float32), _dev(b, torch.float32), precond="factor32")


def test_device_pcg_on_the_trailing_block():
    rows, cols, values, A, n = bs_case()
    bs = np.concatenate([[0], np.cumsum(SIZES)])
    keep = np.arange(bs[6], n)                     # the last four params stay: S is 21 x 21
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES, keep=keep)
    sol, span = pat.solver, pat.keep_span
    d = S.assemble(pat, _dev(values, torch.float64)).clone()
    sol.factorUpTo(d, span)
    inv = pat._to_internal                         # v_internal = v_user[inv]
    Ai = A[inv][:, inv]
    bar = n - len(keep)
    Sc = Ai[bar:, bar:] - Ai[bar:, :bar] @ np.linalg.solve(Ai[:bar, :bar], Ai[:bar, bar:])
    assert np.linalg.cond(Sc) <= 1e3
    b = np.random.default_rng(8).uniform(-1, 1, n - bar)
    bd = _dev(b, torch.float64)
    op, M = pcg.TrailingOperator(sol, d, span), pcg.LowerPrecSolvePrecond(sol, d, span)
    _, st = R.cg_model(n - bar, lambda p: Sc @ p, b, np.float64, _f32_cholesky_precond(Sc), tol=TOL, max_steps=100)
    for ce in (8, None):
        x = torch.full((n - bar,), 7.0, dtype=torch.float64, device="cuda")
        solver = pcg.DevicePCG(M, op, TOL, 100, check_every=ce)
        iters, res = solver.solve(x, bd)
        assert solver.info["stopReason"] == "converged" and res <= TOL
        true_res = np.linalg.norm(b - Sc @ x.cpu().numpy()) / np.linalg.norm(b)
        print("DevicePCG: iterations", iters, "recurrence", res, "true residual", true_res)
        assert true_res <= 2 * TOL
        assert iters <= st["iterations"][0] + 1, (iters, st["iterations"])
    it0, res0 = pcg.PCG(M, op, TOL, 100).solve(torch.zeros_like(x), bd)
    print("PCG: iterations", it0, "residual", res0)
    # plain CG through the same interface: IdentityPrecond takes the kernels' path without a preconditioner
    x = torch.zeros(n - bar, dtype=torch.float64, device="cuda")
    iters, res = pcg.DevicePCG(pcg.IdentityPrecond(), op, TOL, 200).solve(x, bd)
    assert res <= TOL and np.linalg.norm(b - Sc @ x.cpu().numpy()) / np.linalg.norm(b) <= 2 * TOL


def test_gradients_against_solve():
    rows, cols, values, A, n = bs_case()
    kappa = float(np.linalg.cond(A))
    tol = 1e-13
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    rng = np.random.default_rng(6)
    b, w = rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2))
    wd = _dev(w, torch.float64)
    grads = []
    for fn in (lambda v, bb: S.solve(pat, v, bb),
               lambda v, bb: S.solve_cg(pat, v, bb, precond="block_jacobi", tol=tol, max_steps=400)):
        v = _dev(values, torch.float64).requires_grad_(True)
        bb = _dev(b, torch.float64).requires_grad_(True)
        (fn(v, bb) * wd).sum().backward()
        grads.append((v.grad.cpu().numpy(), bb.grad.cpu().numpy()))
    for got, want, name in zip(grads[1], grads[0], ("values", "b")):
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        print("gradient of", name, "relative difference", rel, "bound", 100 * kappa * tol)
        assert rel <= 100 * kappa * tol, (name, rel)


def test_refusals():
    rows, cols, values, A, n = bs_case()
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=SIZES)
    v, b = _dev(values, torch.float64), _dev(np.ones(n), torch.float64)
    with pytest.raises(ValueError, match="precond"):
        S.solve_cg(pat, v, b, precond="ilu")
    with pytest.raises(ValueError, match="x0"):
        S.solve_cg(pat, v, b, x0=torch.zeros(n + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError, match="dtype"):
        S.solve_cg(pat, v, b.float())
    with pytest.raises(ValueError, match="must return a tensor of shape"):
        S.solve_cg(pat, v, b, precond=lambda r: r[:-1])
    wide = [2, 33, 5]
    d = np.arange(40)
    patw = S.SymmetricPattern(d, d, 40, param_sizes=wide)
    with pytest.raises(ValueError, match="param 1 has 33 scalars"):
        S.solve_cg(patw, _dev(np.ones(40), torch.float64), _dev(np.ones(40), torch.float64))
    x = S.solve_cg(patw, _dev(np.full(40, 2.0), torch.float64), _dev(np.ones(40), torch.float64), precond="jacobi")
    assert x.tolist() == [0.5] * 40
    # a callable preconditioner and a start vector
    x0 = torch.from_numpy(np.linalg.solve(A, np.ones(n))).cuda()
    x, i = S.solve_cg(pat, v, b, precond=lambda r: r * 0.5, x0=x0, tol=1e-8, return_info=True)
    assert int(i["iterations"]) <= 1 and int(i["stop"]) == R.CONVERGED
