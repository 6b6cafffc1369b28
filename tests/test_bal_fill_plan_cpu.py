"""CPU: the host plan of the ordered Hessian fill (csrc/bal_fill_plan.cpp through bal.BalFillPlan) against its
own statement -- sorted lists, distinct pairs at the accessor's offsets, chunks that tile the camera lists --
its refusals, and the numpy model of the documented summation order (tests/bal_fill_ref.py) against the
long-double references at the bounds the GPU test uses: the proof, made without a GPU, that the order itself
stays inside the yardstick of the atomic fill."""
import os
import re

import numpy as np
import pytest

import baspacho_amd as B
import bal_fill_ref as F
import bal_ref as R
from baspacho_amd import _lib, bal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bsp_bal_fill_plan_create", "bsp_bal_fill_plan_destroy", "bsp_bal_fill_plan_info",
               "bsp_bal_fill_ordered_f64", "bsp_bal_fill_ordered_f32"]


def _plan(c, obs=None):
    prob = c["prob"]
    oc, op = (prob.obs_cam, prob.obs_pt) if obs is None else obs
    return bal.BalFillPlan(c["sol"], c["cam_size"], prob.num_pts, prob.num_cams, oc, op)


def test_new_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "baspacho_amd_testing.h")) as f:
        thdr = f.read()
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % n, hdr), n
        assert hasattr(lib, n), n
    assert re.search(r"\bint bsp_test_bal_fill_plan\(", thdr) and hasattr(lib, "bsp_test_bal_fill_plan")
    assert callable(bal.DevicePipeline.fill_hessian_ordered) and callable(bal.DevicePipeline.fill_plan)
    import inspect
    assert inspect.signature(bal.lm_optimize_device).parameters["ordered_fill"].default is False


def _check_tables(c, tab, oc, op):
    prob, sol = c["prob"], c["sol"]
    npt, nc = prob.num_pts, prob.num_cams
    oc, op = np.asarray(oc, dtype=np.int64), np.asarray(op, dtype=np.int64)
    kept = np.nonzero((oc >= 0) & (oc < nc) & (op >= 0) & (op < npt))[0]
    assert (tab["kept"], tab["skipped"]) == (len(kept), len(oc) - len(kept))
    assert (tab["numPts"], tab["numCams"], tab["camSize"], tab["C"], tab["W"]) == (npt, nc, c["cam_size"], F.C, F.W)
    # by point: a permutation of the kept observations sorted by (point, camera, index)
    want = kept[np.lexsort((kept, oc[kept], op[kept]))]
    assert np.array_equal(tab["ptObs"], want)
    assert np.array_equal(tab["ptPtr"], np.concatenate([[0], np.cumsum(np.bincount(op[kept], minlength=npt))]))
    # by camera: sorted by (camera, index)
    want = kept[np.lexsort((kept, oc[kept]))]
    assert np.array_equal(tab["camObs"], want)
    assert np.array_equal(tab["camPtr"], np.concatenate([[0], np.cumsum(np.bincount(oc[kept], minlength=nc))]))
    # pairs: the runs of equal (point, camera), distinct, at the host accessor's blocks
    pp = tab["pairPtr"]
    assert pp[0] == 0 and pp[-1] == len(kept) and np.all(np.diff(pp) > 0)
    key = op[tab["ptObs"]] * nc + oc[tab["ptObs"]]
    assert np.array_equal(np.nonzero(np.diff(key))[0] + 1, pp[1:-1])
    assert np.array_equal(tab["pairPt"] * nc + tab["pairCam"], key[pp[:-1]])
    assert len(np.unique(key[pp[:-1]])) == tab["nPairs"]
    for q in range(tab["nPairs"]):
        off, stride, flip = sol.blockOffset(npt + int(tab["pairCam"][q]), int(tab["pairPt"][q]))
        assert (tab["pairOff"][q], tab["pairStride"][q], tab["pairFlip"][q]) == (off, stride, int(flip))
    # diagonal blocks and vector slices
    p2s, ss = sol.paramToSpan(), sol.skel()["spanStart"]
    for p in range(npt):
        assert (tab["ptDiagOff"][p], tab["ptDiagStride"][p]) == tuple(sol.diagBlockOffset(p))
    for k in range(nc):
        assert (tab["camDiagOff"][k], tab["camDiagStride"][k]) == tuple(sol.diagBlockOffset(npt + k))
    assert np.array_equal(tab["ptStart"], ss[p2s[:npt]]) and np.array_equal(tab["camStart"], ss[p2s[npt:]])
    # chunks: consecutive pieces of at most C positions that tile every camera list exactly, full but the last
    assert tab["camChunkPtr"][0] == 0 and tab["camChunkPtr"][-1] == tab["nChunks"]
    for k in range(nc):
        k0, k1 = tab["camChunkPtr"][k], tab["camChunkPtr"][k + 1]
        b, e = tab["chunkBegin"][k0:k1], tab["chunkEnd"][k0:k1]
        n = tab["camPtr"][k + 1] - tab["camPtr"][k]
        assert k1 - k0 == -(-n // F.C) and np.all(tab["chunkCam"][k0:k1] == k)
        if n:
            assert b[0] == tab["camPtr"][k] and e[-1] == tab["camPtr"][k + 1]
            assert np.array_equal(b[1:], e[:-1]) and np.all(e[:-1] - b[:-1] == F.C) and 0 < e[-1] - b[-1] <= F.C
    words = c["cam_size"] * (c["cam_size"] + 1) // 2 + c["cam_size"]
    assert tab["scratchLen"] == tab["nChunks"] * words


@pytest.mark.parametrize("cam_size", [9, 6])
@pytest.mark.parametrize("name", R.FILL_SCENES + ("edges",))
def test_plan_tables(name, cam_size):
    c = F.edge_case(cam_size) if name == "edges" else R.fill_case(name, cam_size)
    plan = _plan(c)
    tab = plan._testTables()
    _check_tables(c, tab, c["prob"].obs_cam, c["prob"].obs_pt)
    info = plan.info()
    assert (info["kept"], info["skipped"], info["pairs"], info["chunks"], info["C"], info["W"], info["scratch_len"],
            info["cam_size"]) == (tab["kept"], 0, tab["nPairs"], tab["nChunks"], F.C, F.W, tab["scratchLen"], cam_size)
    assert info["max_pt_list"] == int(np.diff(tab["ptPtr"]).max())
    assert info["max_cam_list"] == int(np.diff(tab["camPtr"]).max())
    assert info["host_bytes"] > 0 and info["device_bytes"] >= 8 * tab["scratchLen"]
    if name == "dup7":   # seven pairs observed three times
        assert sorted(np.diff(tab["pairPtr"]).tolist())[-8:] == [1] + [3] * 7
    if name == "edges":
        assert np.diff(tab["camPtr"]).tolist() == list(F.EDGE_COUNTS) + [0]
        assert np.diff(tab["camChunkPtr"]).tolist() == [1, 1, 1, 1, 1, 2, 3, 0]
        assert tab["ptPtr"][-1] == tab["ptPtr"][-2] and int(np.diff(tab["ptPtr"]).max()) == 7


@pytest.mark.parametrize("cam_size", [9, 6])
def test_out_of_range_observations_are_counted_and_listed_nowhere(cam_size):
    c = R.fill_case("30x8", cam_size)
    oc, op, _, _, _, skipped = F.with_bad_observations(c)
    tab = _plan(c, (oc, op))._testTables()
    assert (tab["kept"], tab["skipped"]) == (len(oc) - 9, 9)
    bad = set(np.nonzero(skipped)[0].tolist())
    assert not bad & set(tab["ptObs"].tolist()) and not bad & set(tab["camObs"].tolist())
    _check_tables(c, tab, oc, op)
    # the same pairs and lists as the clean list, under the shifted observation indices
    clean = _plan(c)._testTables()
    shift = np.nonzero(~skipped)[0]
    assert np.array_equal(tab["ptObs"], shift[clean["ptObs"]]) and np.array_equal(tab["camObs"], shift[clean["camObs"]])
    for k in ("pairPtr", "pairOff", "pairFlip", "chunkBegin", "chunkEnd"):
        assert np.array_equal(tab[k], clean[k]), k


def test_refusals():
    c = R.fill_case("30x8", 9)
    prob, sol = c["prob"], c["sol"]
    npt, nc = prob.num_pts, prob.num_cams
    one = np.zeros(1, dtype=np.int64)
    with pytest.raises(RuntimeError, match=r"2\^31"):   # refused before the lists are read
        bal.BalFillPlan(sol, 9, npt, nc, one, one, num_obs=2 ** 31)
    with pytest.raises(RuntimeError, match=r"2\^31"):
        bal.BalFillPlan(sol, 9, npt, nc, one, one, num_obs=-1)
    with pytest.raises(RuntimeError, match="camera size must be 9 or 6"):
        bal.BalFillPlan(sol, 7, npt, nc, one, one)
    with pytest.raises(RuntimeError, match="has size 9, the BAL layout needs 6"):
        bal.BalFillPlan(sol, 6, npt, nc, prob.obs_cam, prob.obs_pt)
    with pytest.raises(RuntimeError, match="has size 6, the BAL layout needs 9"):
        bal.BalFillPlan(R.fill_case("30x8", 6)["sol"], 9, npt, nc, prob.obs_cam, prob.obs_pt)
    with pytest.raises(RuntimeError, match="parameters"):
        bal.BalFillPlan(sol, 9, npt + 1, nc, prob.obs_cam, prob.obs_pt)
    with pytest.raises(RuntimeError, match="has size"):   # the same number of parameters, split elsewhere
        bal.BalFillPlan(sol, 9, npt + 1, nc - 1, prob.obs_cam, prob.obs_pt)
    # a pair the structure does not hold (the points of 16x400 are eliminated first, so a camera-point block
    # exists only where the camera sees the point)
    c2 = R.fill_case("16x400", 9)
    p2 = c2["prob"]
    cam = int(np.setdiff1d(np.arange(p2.num_cams), p2.obs_cam[p2.obs_pt == 7])[0])
    with pytest.raises(RuntimeError, match="observation 1: the block of camera %d and point 7 is not" % cam):
        bal.BalFillPlan(c2["sol"], 9, p2.num_pts, p2.num_cams, np.array([p2.obs_cam[0], cam]),
                        np.array([p2.obs_pt[0], 7]))
    # the C entry refuses NULL arguments and a plan of another solver before any launch (no GPU is touched)
    import ctypes
    lib = _lib.load()
    plan = _plan(c)
    other = R.fill_case("9x9", 9)["sol"]
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(8)
    lam = ctypes.c_double(0.0)
    for args, msg in (((None, plan._h, p, p, p, lam, p, null, null), "solver is NULL"),
                      ((sol._h, None, p, p, p, lam, p, null, null), "plan is NULL"),
                      ((other._h, plan._h, p, p, p, lam, p, null, null), "another solver"),
                      ((sol._h, plan._h, p, p, p, lam, null, null, null), "data is NULL"),
                      ((sol._h, plan._h, null, p, p, lam, p, null, null), "Jc, Jp or res is NULL"),
                      ((sol._h, plan._h, p, p, null, lam, p, null, null), "Jc, Jp or res is NULL")):
        assert lib.bsp_bal_fill_ordered_f64(*args) != 0
        assert msg in lib.bsp_last_error().decode(), msg
    assert lib.bsp_bal_fill_plan_info(None, (ctypes.c_int64 * 12)()) != 0


# ---- the model against the long-double references --------------------------------------------------------
def _model_against(c, exp, dtype, lam, seed, what):
    tab = _plan(c)._testTables()
    prior = R.prior_for(exp, dtype, seed=seed)
    diag = c["lay"]["diag"]
    got, gotg = F.model_fill(tab, c["Jc"], c["Jp"], c["res"], prior, dtype, lam, diag)
    F.check_fill(diag, dtype, exp, prior, got, gotg, lam, what)
    return tab, prior, got, gotg


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("cam_size", [9, 6])
@pytest.mark.parametrize("name", R.FILL_SCENES)
def test_model_meets_the_bounds_of_the_dense_reference(name, cam_size, dtype):
    c = R.fill_case(name, cam_size)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    for lam in (0.0, 0.3):
        _model_against(c, exp, dtype, lam, len(name) + cam_size, (name, cam_size, lam))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("cam_size", [9, 6])
def test_model_meets_the_bounds_on_the_boundary_scene(cam_size, dtype):
    c = F.edge_case(cam_size)
    prob = c["prob"]
    exp = F.blockwise_expected(prob.num_pts, prob.num_cams, cam_size, prob.obs_cam, prob.obs_pt, c["Jc"], c["Jp"],
                               c["res"], c["lay"], dtype)
    for lam in (0.0, 0.3):
        tab, prior, got, gotg = _model_against(c, exp, dtype, lam, 21 + cam_size, ("edges", cam_size, lam))
    # the camera and the point that nobody observes move by damping only
    from known_factor import bitwise_equal
    lay = c["lay"]
    alone = np.concatenate([3 * (prob.num_pts - 1) + np.arange(3),
                            3 * prob.num_pts + cam_size * (prob.num_cams - 1) + np.arange(cam_size)])
    mine = np.isin(lay["rows"], alone) | np.isin(lay["cols"], alone)
    assert mine.any() and not exp["Htouched"][mine].any() and not exp["gtouched"][lay["vec"][alone]].any()
    got0, gotg0 = F.model_fill(tab, c["Jc"], c["Jp"], c["res"], prior, dtype, 0.0, lay["diag"])
    assert bitwise_equal(got0[mine], prior[0][mine]) and bitwise_equal(gotg0[lay["vec"][alone]], prior[1][lay["vec"][alone]])
    off = mine.copy()
    off[lay["diag"]] = False
    assert bitwise_equal(got[off], prior[0][off])
    assert not bitwise_equal(got[lay["diag"][alone]], prior[0][lay["diag"][alone]])


def test_blockwise_reference_is_the_dense_reference():
    """on a scene that has both: the same touched elements and counts, sums equal to long-double rounding"""
    for name, cs in (("37x5", 9), ("dup7", 6)):
        c = R.fill_case(name, cs)
        prob = c["prob"]
        a = R.expected_fill(c["ne"], c["lay"], np.float64)
        b = F.blockwise_expected(prob.num_pts, prob.num_cams, cs, prob.obs_cam, prob.obs_pt, c["Jc"], c["Jp"], c["res"],
                                 c["lay"], np.float64)
        tiny = 64 * np.finfo(np.longdouble).eps
        for k in ("Htouched", "gtouched"):
            assert np.array_equal(a[k], b[k]), k
        for k, s in (("H", "HA"), ("HA", "HA"), ("Hbound", "Hbound"), ("g", "gA"), ("gA", "gA"), ("gbound", "gbound")):
            assert np.all(np.abs(a[k] - b[k]) <= tiny * np.abs(a[s])), k


def test_model_is_an_order_not_a_set():
    """the model's bits depend on the order: the same observations listed backwards give other bits somewhere
    (so a bitwise comparison with it does pin the order), yet the same values to the bound"""
    c = R.fill_case("16x400", 9)
    prob = c["prob"]
    exp = R.expected_fill(c["ne"], c["lay"], np.float64)
    prior = R.prior_for(exp, np.float64, seed=3)
    tab = _plan(c)._testTables()
    a, ag = F.model_fill(tab, c["Jc"], c["Jp"], c["res"], prior, np.float64, 0.0)
    rev = np.arange(len(prob.obs_cam))[::-1]
    tabr = _plan(c, (prob.obs_cam[rev], prob.obs_pt[rev]))._testTables()
    b, bg = F.model_fill(tabr, c["Jc"][rev], c["Jp"][rev], c["res"][rev], prior, np.float64, 0.0)
    assert not np.array_equal(a, b)
    F.check_fill(c["lay"]["diag"], np.float64, exp, prior, b, bg, 0.0, "reversed list")
