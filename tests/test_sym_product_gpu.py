"""GPU: products with a symmetric matrix given as entries on the MI355X, solver level.
SymProduct.mv and .outer must be bitwise the numpy statements (sym_product_ref.py) in f64 and f32 on every
case, for q in {1, 2, 3, 16, 17} vectors and batches of {1, 2, 5}, on buffers that start at odd element
offsets between guard bands (buffer_edges.framed), into outputs full of the sentinel NaN; batch members
bitwise the single call; two runs the same bits; every refusal raised before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import baspacho_amd as B
from buffer_edges import SENTINEL, framed, is_sentinel
import sym_product_ref as R

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
QS = [1, 2, 3, 16, 17]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dev(a, npdt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(npdt))).cuda()


def _framed_call(npdt, ins, out_shape, call):
    """call(*inputs, out) with every tensor a payload of one frame: inputs bitwise untouched, guards intact,
    out (full of the sentinel before) fully written.  Returns the host copy of out"""
    fr = framed(npdt, list(ins) + [np.full(int(np.prod(out_shape)), SENTINEL[npdt], dtype=npdt)])
    assert is_sentinel(fr.host(len(ins))).all()
    args = [fr.view(k).view(h.shape) for k, h in enumerate(ins)]
    out = fr.view(len(ins)).view(tuple(out_shape))
    assert all(a.data_ptr() % 16 != 0 for a in args + [out] if a.numel())
    ret = call(*args, out)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr()
    fr.assert_intact(read_only=range(len(ins)))
    got = fr.host(len(ins)).reshape(out_shape)
    assert not is_sentinel(got).any(), "%d elements of out were not written" % int(is_sentinel(got).sum())
    return got


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", R.CASES)
def test_mv_bitwise(name, dt):
    _, npdt = DT[dt]
    c, prod = R.case(name), R.pattern(name).product
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    rng = np.random.default_rng(31)
    v = c["values"].astype(npdt)
    empty = np.diff(R.row_terms(n, rows, cols, tri)[0]) == 0
    for q in [None] + QS:
        x = rng.uniform(-1, 1, (n,) if q is None else (n, q)).astype(npdt)
        want = R.mv_model(n, rows, cols, tri, v, x, npdt)
        got = _framed_call(npdt, [v, x], x.shape, lambda a, b, o: prod.mv(a, b, out=o))
        assert _bits_equal(got, want), (name, dt, q)
        rows_empty = got.reshape(n, -1)[empty]
        assert not rows_empty.any() and not np.signbit(rows_empty).any()
        again = prod.mv(_dev(v, npdt), _dev(x, npdt)).cpu().numpy()
        assert _bits_equal(again, got), "two runs differ"


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["dups", "full", "blocks", "arrow65", "arrow129", "empty"])
def test_mv_batches_bitwise(name, dt):
    _, npdt = DT[dt]
    c, prod = R.case(name), R.pattern(name).product
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    rng = np.random.default_rng(32)
    for nb, q in ((1, 3), (2, None), (2, 17), (5, 1), (5, 16)):
        v = rng.uniform(-1, 1, (nb, len(rows))).astype(npdt)
        x = rng.uniform(-1, 1, (nb, n) if q is None else (nb, n, q)).astype(npdt)
        got = _framed_call(npdt, [v, x], x.shape, lambda a, b, o: prod.mv(a, b, out=o))
        for b in range(nb):
            assert _bits_equal(got[b], R.mv_model(n, rows, cols, tri, v[b], x[b], npdt)), (name, dt, nb, q, b)
            one = prod.mv(_dev(v[b], npdt), _dev(x[b], npdt)).cpu().numpy()
            assert _bits_equal(one, got[b]), "member %d is not the single call" % b


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", R.CASES)
def test_outer_bitwise(name, dt):
    _, npdt = DT[dt]
    c, prod = R.case(name), R.pattern(name).product
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    nnz = len(rows)
    keep = rows >= cols
    rng = np.random.default_rng(33)
    for q in [None] + QS:
        g = rng.uniform(-1, 1, (n,) if q is None else (n, q)).astype(npdt)
        x = rng.uniform(-1, 1, g.shape).astype(npdt)
        want = R.outer_model(n, rows, cols, tri, g, x, npdt)
        got = _framed_call(npdt, [g, x], (nnz,), lambda a, b, o: prod.outer(a, b, out=o))
        assert _bits_equal(got, want), (name, dt, q)
        assert not got[~keep].any() and not np.signbit(got[~keep]).any()
        key = rows[keep] * n + cols[keep]
        for k in np.unique(key):  # every duplicate holds the full value
            assert len(set(got[keep][key == k].tolist())) == 1
        assert _bits_equal(prod.outer(_dev(g, npdt), _dev(x, npdt)).cpu().numpy(), got), "two runs differ"
    for nb, q in ((1, 2), (2, None), (5, 3)):
        g = rng.uniform(-1, 1, (nb, n) if q is None else (nb, n, q)).astype(npdt)
        x = rng.uniform(-1, 1, g.shape).astype(npdt)
        got = _framed_call(npdt, [g, x], (nb, nnz), lambda a, b, o: prod.outer(a, b, out=o))
        for b in range(nb):
            assert _bits_equal(got[b], R.outer_model(n, rows, cols, tri, g[b], x[b], npdt)), (name, dt, nb, q, b)
            assert _bits_equal(prod.outer(_dev(g[b], npdt), _dev(x[b], npdt)).cpu().numpy(), got[b])
        assert _bits_equal(prod.outer(_dev(g, npdt), _dev(x, npdt), batched=True).cpu().numpy(), got)


def test_refusals_before_any_launch():
    c, pat = R.case("dups"), R.pattern("dups")
    prod, sol, n, nnz = pat.product, pat.solver, c["n"], len(c["rows"])
    lib = sol._lib
    tdt = torch.float64
    v = torch.rand(nnz, dtype=tdt, device="cuda")
    x = torch.rand(n, 2, dtype=tdt, device="cuda")
    nan = float("nan")
    out = torch.full((n, 2), nan, dtype=tdt, device="cuda")
    gout = torch.full((nnz,), nan, dtype=tdt, device="cuda")
    P = ctypes.c_void_p

    def raw(fn, *args):
        rc = getattr(lib, fn)(sol._h, prod._h, *args)
        return rc, lib.bsp_last_error().decode()

    def arr(*ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])

    q2, q0 = ctypes.c_int64(2), ctypes.c_int64(0)
    # q < 1
    rc, msg = raw("bsp_sym_product_mv_f64", P(v.data_ptr()), P(x.data_ptr()), q0, P(out.data_ptr()))
    assert rc != 0 and "q = 0" in msg
    rc, msg = raw("bsp_sym_product_outer_f64", P(x.data_ptr()), P(x.data_ptr()), ctypes.c_int64(-1), P(gout.data_ptr()))
    assert rc != 0 and "q = -1" in msg
    # NULL member, NULL array, empty batch
    rc, msg = raw("bsp_sym_product_mv_f64", P(v.data_ptr()), None, q2, P(out.data_ptr()))
    assert rc != 0 and "NULL" in msg
    rc, msg = raw("bsp_sym_product_mv_f64", None, P(x.data_ptr()), q2, P(out.data_ptr()))
    assert rc != 0 and "values pointer of batch member 0 is NULL" in msg
    rc, msg = raw("bsp_sym_product_mv_f64", P(v.data_ptr()), P(x.data_ptr()), q2, None)
    assert rc != 0 and "NULL" in msg
    rc, msg = raw("bsp_sym_product_mv_batched_f64", None, arr(x), q2, arr(out), ctypes.c_int32(1))
    assert rc != 0 and "NULL" in msg
    rc, msg = raw("bsp_sym_product_mv_batched_f64", arr(v), arr(x), q2, arr(out), ctypes.c_int32(0))
    assert rc != 0 and "empty" in msg
    rc, msg = raw("bsp_sym_product_outer_batched_f64", arr(x, None), arr(x, x), q2, arr(gout, gout.clone()),
                  ctypes.c_int32(2))
    assert rc != 0 and "batch member 1 is NULL" in msg
    # a repeated output pointer
    rc, msg = raw("bsp_sym_product_mv_batched_f64", arr(v, v), arr(x, x), q2, arr(out, out), ctypes.c_int32(2))
    assert rc != 0 and "repeats" in msg
    # an output that aliases an input: its own, partially, and another member's
    rc, msg = raw("bsp_sym_product_mv_f64", P(v.data_ptr()), P(x.data_ptr()), q2, P(x.data_ptr()))
    assert rc != 0 and "aliases its vector" in msg
    rc, msg = raw("bsp_sym_product_mv_f64", P(v.data_ptr()), P(x.data_ptr()), q2, P(x.data_ptr() + 8 * (2 * n - 1)))
    assert rc != 0 and "aliases its vector" in msg
    rc, msg = raw("bsp_sym_product_outer_f64", P(gout.data_ptr()), P(x.data_ptr()), ctypes.c_int64(1), P(gout.data_ptr()))
    assert rc != 0 and "aliases its gradient" in msg
    out2 = out.clone()
    rc, msg = raw("bsp_sym_product_mv_batched_f64", arr(v, v), arr(x, out), q2, arr(out, out2), ctypes.c_int32(2))
    assert rc != 0 and "also an output" in msg
    # a map built on another solver
    other = R.pattern("full")
    assert other.solver.order() == n
    rc = lib.bsp_sym_product_mv_f64(other.solver._h, prod._h, P(v.data_ptr()), P(x.data_ptr()), q2, P(out.data_ptr()))
    assert rc != 0 and "another solver" in lib.bsp_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(gout).all() and torch.isnan(out2).all(), "a refused call launched"
    # the Python layer: shapes, dtypes, devices
    with pytest.raises(ValueError, match="values must be"):
        prod.mv(v[:-1], x)
    with pytest.raises(ValueError, match="x must be"):
        prod.mv(v, x[:-1])
    with pytest.raises(ValueError, match="x must be"):
        prod.mv(v.expand(2, nnz).contiguous(), x)
    with pytest.raises(TypeError, match="x is"):
        prod.mv(v, x.float())
    with pytest.raises(TypeError):
        prod.mv(v.half(), x.half())
    with pytest.raises(ValueError, match="out must be"):
        prod.mv(v, x, out=out[:, :1])
    with pytest.raises(ValueError, match="g has shape"):
        prod.outer(x, x[:, :1])
    with pytest.raises(ValueError, match="device memory"):
        prod.mv(v.cpu(), x.cpu())
    with pytest.raises(ValueError, match="empty batch"):
        prod.mv(v.new_zeros((0, nnz)), x.new_zeros((0, n)))
    with pytest.raises(TypeError, match="torch.Tensor"):
        prod.mv(v.cpu().numpy(), x)
    # and a valid call still works afterwards
    want = R.mv_model(n, c["rows"], c["cols"], c["triangle"], v.cpu().numpy(), x.cpu().numpy(), np.float64)
    assert _bits_equal(prod.mv(v, x, out=out).cpu().numpy(), want)
    assert isinstance(prod, B.SymProduct)
