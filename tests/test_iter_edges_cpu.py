"""CPU: the host side of the buffer-edge tests of the CG and Lanczos pieces (tests/test_iter_edges_gpu.py): the
documented layout of the two work areas, restated here and compared with bsp_cg_work_bytes and
bsp_lanczos_work_bytes (which run on the host); the write-set table of tests/iter_driver.py against the pieces
the public header exports; the 16-byte-aligned payloads of buffer_edges.Frame.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

import buffer_edges as BE
import iter_driver as D
import sym_product_ref as SP
from buffer_edges import Frame, SENTINEL_BITS

NS, QS, KS = (0, 1, 1024, 1025), (1, 3), (1, 8, 9)


def _parts(n):
    return max((n + 1023) // 1024, 1)


def _up16(b):
    return (b + 15) // 16 * 16


def test_work_bytes_are_the_documented_layout():
    sol = SP.pattern("blocks").solver
    for n in NS:
        for q in QS:
            # CG: q columns of `parts` 16-byte partials, then n 4-byte bad-pivot words rounded up to 16 bytes
            assert D.work_bytes(sol, "cg", n, q) == 16 * q * _parts(n) + _up16(4 * max(n, 1)), (n, q)
            for kmax in KS:
                # Lanczos: kmax sums of q columns of `parts` partials, then q kmax 8-byte projection coefficients
                want = 16 * q * kmax * _parts(n) + _up16(8 * q * kmax)
                assert D.work_bytes(sol, "lanczos", n, q, kmax) == want, (n, q, kmax)
    # the cases the GPU tests lean on: a bad-pivot area that is no multiple of 16 bytes, an odd count of coefficients
    assert (4 * 1025) % 16 != 0 and D.work_bytes(sol, "cg", 1025, 1) == 32 + 4112
    assert (8 * 1 * 9) % 16 != 0 and D.work_bytes(sol, "lanczos", 1, 1, 9) == 144 + 80


def test_the_write_set_table_names_every_exported_piece():
    exported = D.exported_pieces()
    assert len(exported) >= 18, exported
    for must in ("cg_init", "cg_precond_build", "lanczos_subtract", "lanczos_work_bytes"):
        assert must in exported, "the header parse lost %s" % must
    missing = [p for p in exported if p not in D.WRITE_SETS]
    assert not missing, "pieces of include/baspacho_amd.h without a row in iter_driver.WRITE_SETS: %s" % missing
    stale = [p for p in D.WRITE_SETS if p not in exported]
    assert not stale, "rows of iter_driver.WRITE_SETS that the header no longer exports: %s" % stale
    cg_ops = {"b", "x", "r", "p", "ap", "z", "minv", "values", "state", "status", "work"}
    lz_ops = {"v0", "w", "basis", "slot", "coef", "state", "work"}
    for piece, row in D.WRITE_SETS.items():
        sets = list(row["writes"].values()) if isinstance(row["writes"], dict) else [row["writes"]]
        for s in sets + [row.get("fold", ())]:
            assert set(s) <= (cg_ops if piece.startswith("cg_") else lz_ops), (piece, s)
        assert set(row.get("columns", ())) <= set().union(*map(set, sets)), piece
    # read-only by declaration: b, p, Ap and the values in alpha; minv, the start vector, z of kind 0
    assert D.write_set("cg_alpha") == ("state", "work")
    assert "z" not in D.write_set("cg_precond", kind=0) and "z" in D.write_set("cg_precond", kind=2)
    assert D.write_set("cg_direction") == ("p",)
    assert "coef" not in D.write_set("lanczos_update") and "coef" in D.write_set("lanczos_update", fold=True)
    assert all("v0" not in D.write_set(p) and "basis" not in D.write_set(p) for p in D.WRITE_SETS
               if p.startswith("lanczos_") and not isinstance(D.WRITE_SETS[p]["writes"], dict))


def test_the_driver_touches_no_gpu_at_import():
    assert not hasattr(D, "torch"), "iter_driver works on the tensors and addresses it is handed; it needs no torch"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_aligned_payloads_of_a_frame(dtype):
    sizes = [1, 6, 257, 0, 1030]
    fr = Frame(sizes, dtype, guard=33, device="cpu", align_bytes=16)
    item = np.dtype(dtype).itemsize
    at = 0
    for k, s in enumerate(sizes):
        v = fr.view(k)
        assert v.numel() == s and fr.offsets[k] - at >= 33, "payload %d has a short guard in front" % k
        assert (fr.base.data_ptr() + fr.offsets[k] * item) % 16 == 0, "payload %d is not 16-byte aligned" % k
        if s:
            assert v.data_ptr() % 16 == 0
        at = fr.offsets[k] + s
    assert fr.total - at >= 33
    fr.assert_intact()
    for k, s in enumerate(sizes):
        fr.fill(k, np.arange(s, dtype=dtype) + k)
    fr.seal().assert_intact(read_only=range(len(sizes)))
    np.testing.assert_array_equal(fr.host(2), np.arange(257, dtype=dtype) + 2)
    # one word behind the last own word of a payload is foreign
    fr.base[fr.offsets[4] + sizes[4]] = 1.0
    with pytest.raises(AssertionError, match="outside the payloads"):
        fr.assert_intact()
    fr2 = Frame([4], dtype, guard=8, device="cpu", align_bytes=16)
    fr2.seal()
    fr2.view(0)[3] = 2.0
    with pytest.raises(AssertionError, match="read-only operand"):
        fr2.assert_intact(read_only=[0])
    with pytest.raises(AssertionError):
        Frame([4], dtype, device="cpu", align_bytes=item + 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_default_layout_of_a_frame_is_unchanged(dtype):
    """the layout every earlier buffer-edge test was written against, restated: guard words, then one more where
    the offset would be even, the payload, ...; a trailing guard; all of it the sentinel"""
    sizes, guard = [3, 8, 0, 5], 10
    fr = Frame(sizes, dtype, guard=guard, device="cpu")
    want, at = [], 0
    for s in sizes:
        at += guard
        if at % 2 == 0:
            at += 1
        want.append(at)
        at += s
    assert fr.offsets == want == [11, 25, 43, 53] and fr.total == at + guard == 68 and fr.align_bytes is None
    assert fr.base.numel() == 68 and fr.base.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    assert bool((BE._bits(fr.base) == SENTINEL_BITS[np.dtype(dtype)]).all())
    same = Frame(sizes, dtype, guard=guard, device="cpu", align_bytes=None)
    assert same.offsets == fr.offsets and same.total == fr.total
