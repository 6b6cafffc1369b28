"""CPU: the host plan of the block diagonal of S ("schur_jacobi") against the numpy restatement
(schur_jacobi_ref.py) on schur_ref's cases and the case of the chunk and pseudo-pair edges; every refusal with its
message; and the restatement alone: the blocks before inversion against the dense C - F^T B^-1 F, and the
preconditioned conjugate gradient on S against the dense solution of the damped normal equations."""
import ctypes
import re

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import sparse as S

import cgls_ref as C
import schur_jacobi_ref as J
import schur_ref as SR

NAMES = ("bsp_jac_schur_sjacobi_info", "bsp_jac_schur_sjacobi_table", "bsp_jac_schur_kept_plan_built") + tuple(
    "bsp_jac_schur_sjacobi_%s_%s%s" % (op, b, sfx) for op in ("build", "apply") for b in ("", "batched_")
    for sfx in ("f64", "f32"))
TABLES = ("block_pair", "block_chunk", "block_width", "block_off", "chunk_pair", "chunk_block", "chunk_part", "pair_elim",
          "pair_row", "pair_rec", "row_of", "rec")


def test_symbols_are_declared_and_exported():
    import os
    lib = B._lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(B.__file__))), "include",
                               "baspacho_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("schurJacobiInfo", "schurJacobiTable", "schurJacobiBuild", "schurJacobiApply"):
        assert callable(getattr(B.JacobianSchur, name))


@pytest.mark.parametrize("name", J.CASES)
def test_every_table_matches_the_restatement(name):
    c, elim, jop, sch = J.operator(name)
    want, got = J.plan(name), sch.map.schurJacobiTable()
    assert set(got) == set(TABLES)
    for key in TABLES:
        wide = key in ("block_off", "chunk_part")
        assert got[key].dtype == (np.int64 if wide else np.int32) and np.array_equal(got[key], want[key]), (name, key)
    info = sch.map.schurJacobiInfo()
    pseudo = int((want["pair_elim"] < 0).sum())
    assert info["blocks"] == len(want["block_width"]) and info["pseudo_pairs"] == pseudo
    assert info["real_pairs"] == len(want["pair_elim"]) - pseudo and info["pair_rows"] == len(want["row_of"])
    assert info["chunks"] == len(want["chunk_block"]) and info["inverse_elems"] == int(want["block_off"][-1])
    assert info["partial_elems"] == int(want["chunk_part"][-1])
    words = sum(len(want[k]) for k in TABLES if k not in ("block_off", "chunk_part", "row_of", "block_width"))
    words += 2 * len(want["block_width"]) + (len(want["block_width"]) + 1) + sch.nK  # widths, firsts, starts, scalar -> block
    assert info["device_bytes"] == 4 * words + 8 * (len(want["block_off"]) + len(want["chunk_part"]))
    # the order: the pairs of a block in ascending eliminated param, the pseudo-pairs behind them; rows ascending
    for b in range(info["blocks"]):
        e = want["pair_elim"][want["block_pair"][b]:want["block_pair"][b + 1]].astype(np.int64)
        real = e[e >= 0]
        assert (np.diff(real) > 0).all() and (e[len(real):] < 0).all()
    for p in range(len(want["pair_elim"])):
        assert (np.diff(want["row_of"][want["pair_row"][p]:want["pair_row"][p + 1]]) > 0).all()
    assert (np.diff(want["chunk_pair"]) <= J.CHUNK).all() and (np.diff(want["chunk_pair"]) > 0).all()


def test_the_edges_case_has_the_edges_it_is_for():
    t = J.plan("edges")
    pairs = np.diff(t["block_pair"])
    real = [int((t["pair_elim"][t["block_pair"][b]:t["block_pair"][b + 1]] >= 0).sum()) for b in range(len(pairs))]
    assert real == [63, 64, 65, 129, 0, 0, 0, 0, 0]
    assert (pairs - real).tolist() == [0, 0, 0, 0, 1, 1, 2, 3, 0]  # pseudo-pairs of 1, 64, 65 and 130 free rows
    assert np.diff(t["block_chunk"]).tolist() == [1, 1, 2, 3, 1, 1, 1, 1, 0]
    assert t["block_width"].tolist() == [32, 1, 3, 2, 2, 2, 2, 2, 2]
    rows = np.diff(t["pair_row"])
    assert rows.max() == 130 and rows.min() == 1
    pseudo_rows = rows[t["pair_elim"] < 0]
    assert pseudo_rows.tolist() == [1, 64, 64, 1, 64, 64, 2]
    assert (t["rec"] < 0).any()  # records with absent entries
    mdl, pc = J.model("edges", np.float64, False)
    assert mdl.status.tolist() == [int(mdl.t["elim_scalar"][-1]), 1]  # the zero-valued eliminated param is bad
    assert (mdl.binv[mdl.block_off[-2]:] == 0).all()
    first = int(t["kept_first"][-1])
    assert pc.status.tolist() == [first, 1] and (pc.minv[t["block_off"][-2]:] == 0).all()  # the block without rows
    assert J.model("edges", np.float64, True)[1].status.tolist() == [-1, 0]


# ---- refusals -----------------------------------------------------------------------------------------------
def test_refusals():
    lib = B._lib.load()
    c, elim, jop, sch = J.operator("w1")
    out = (ctypes.c_int64 * 8)()
    assert lib.bsp_jac_schur_sjacobi_info(None, out) != 0
    assert "bsp_jac_schur_sjacobi_info: NULL argument" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_info(sch.map._h, None) != 0
    assert lib.bsp_jac_schur_sjacobi_table(None, ctypes.c_int32(0), None, None, None, None) != 0
    assert "bsp_jac_schur_sjacobi_table: the map is NULL" in lib.bsp_last_error().decode()
    for part in (-1, 4):
        assert lib.bsp_jac_schur_sjacobi_table(sch.map._h, ctypes.c_int32(part), None, None, None, None) != 0
        assert "bsp_jac_schur_sjacobi_table: unknown part %d" % part in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_table(sch.map._h, ctypes.c_int32(2), None, None, None, None) != 0
    assert "an output array is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_kept_plan_built(None, None) != 0
    # the existing entries keep refusing what they refused
    five = (ctypes.c_int64 * 5)()
    assert lib.bsp_jac_schur_precond_info(sch.map._h, ctypes.c_int32(3), five) != 0
    assert "unknown kind 3" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_table(sch.map._h, ctypes.c_int32(10), None, None, None, None) != 0
    assert "unknown part 10" in lib.bsp_last_error().decode()
    with pytest.raises(ValueError, match="kind must be 'jacobi' or 'block_jacobi'"):
        sch.map.precondInfo("schur_jacobi")
    # a kept param wider than 32, by name, from the plan and from lstsq_cg before any device work
    wide = S.JacobianOperator([0, 1], [0, 40], 2, 42, param_sizes=[8, 33, 1])
    with pytest.raises(RuntimeError, match=r"jacobian schur: kept param 1 has 33 scalars; schur_jacobi takes params of at "
                                           r"most 32"):
        S.JacobianSchur(wide, [0]).map.schurJacobiInfo()
    # the device entries check their operands before any device work
    sol, h, q1 = jop.solver._h, sch.map._h, ctypes.c_int64(1)
    assert lib.bsp_jac_schur_sjacobi_build_f64(None, h, None, None, None, None, None, None, None) != 0
    assert "the solver is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_build_f64(sol, None, None, None, None, None, None, None, None) != 0
    assert "the map is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_apply_f32(sol, None, q1, None, None, None, None, None) != 0
    assert "the map is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_build_f64(sol, h, None, None, None, None, None, None, None) != 0
    assert "schurJacobiBuild: the workspace pointer is NULL" in lib.bsp_last_error().decode()
    work = ctypes.c_void_p(4096)  # (never dereferenced: the checks come first)
    assert lib.bsp_jac_schur_sjacobi_build_f64(sol, h, None, None, None, None, None, ctypes.c_void_p(4097), None) != 0
    assert "schurJacobiBuild: the workspace is not 16-byte aligned" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_build_f64(sol, h, None, None, None, None, None, work, None) != 0
    assert "schurJacobiBuild: the status pointer is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_build_f32(sol, h, None, None, None, None, None, work, work) != 0
    assert "schurJacobiBuild: the values pointer of batch member 0 is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_build_batched_f64(sol, h, None, None, None, None, None, work, work,
                                                       ctypes.c_int32(0)) != 0
    assert "schurJacobiBuild: the batch is empty" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_apply_f64(sol, h, ctypes.c_int64(0), None, None, None, work, work) != 0
    assert "schurJacobiApply" in lib.bsp_last_error().decode() and "q" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_apply_f64(sol, h, q1, None, None, None, work, None) != 0
    assert "schurJacobiApply: the state pointer is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_apply_batched_f64(sol, h, q1, None, None, None, work, work, ctypes.c_int32(-1)) != 0
    assert "schurJacobiApply: the batch is empty" in lib.bsp_last_error().decode()
    other = S.JacobianOperator([0], [0], 1, 1)
    assert lib.bsp_jac_schur_sjacobi_apply_f64(other.solver._h, h, q1, None, None, None, work, work) != 0
    assert "schurJacobiApply: the map was built on another solver" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_sjacobi_build_f64(other.solver._h, h, None, None, None, None, None, work, work) != 0
    assert "schurJacobiBuild: the map was built on another solver" in lib.bsp_last_error().decode()


def test_the_plan_does_not_build_the_kept_item_plan():
    c, elim = SR.case("w8")
    jop = S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
    sch = S.JacobianSchur(jop, np.asarray(elim, dtype=np.int64))
    before = sch.map.info()
    assert sch.map.schurJacobiInfo()["kept_item_plan_built"] is False
    sch.map.schurJacobiTable()
    assert sch.map.schurJacobiInfo()["kept_item_plan_built"] is False and sch.map.info() == before
    sch.map.precondInfo("block_jacobi")
    assert sch.map.schurJacobiInfo()["kept_item_plan_built"] is True


# ---- the restatement alone ----------------------------------------------------------------------------------
def roundings(t):
    """k of the bound: the roundings on the longest path to an element of A_b.  F[l, c]: one per product and one per
    addition over the R rows of a pair, R + 1 at most on a path (the fold from +0 adds exactly first); Y: w_e + 1; E:
    w_e + 1; W: 1 (G's own path, R + 1, is shorter); P: the pairs of a chunk, at most 64 additions; A: the chunks;
    d: 1"""
    rows = int(np.diff(t["pair_row"]).max())
    we = max(w for _, w in t["widths"])
    return (rows + 1) + 2 * (we + 1) + 1 + min(J.CHUNK, int(np.diff(t["block_pair"]).max())) \
        + int(np.diff(t["block_chunk"]).max()) + 1


@pytest.mark.parametrize("name", J.CASES)
@pytest.mark.parametrize("damped", [False, True])
def test_the_blocks_are_those_of_the_dense_reduced_matrix(name, damped):
    """|A_b - S_bb| <= gamma_k (|C_bb| + |F|^T |Binv| |F|)_bb elementwise on the lower triangle, in float64"""
    mdl, pc = J.model(name, np.float64, damped)
    t = J.plan(name)
    k = roundings(t)
    u = 2.0 ** -53
    gamma = k * u / (1 - k * u)
    worst = 0.0
    for b, (A, (Sd, absb)) in enumerate(zip(pc.blocks, J.dense_blocks(mdl, t))):
        lo = np.tril_indices(A.shape[0])
        err, bound = np.abs(A - Sd)[lo], gamma * absb[lo]
        assert (err <= bound).all(), (name, b, (err / np.maximum(bound, 1e-300)).max())
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print("%s damped=%s: k = %d, largest |A - S| / bound = %.3g" % (name, damped, k, worst))


TOL = 1e-12


@pytest.mark.parametrize("name", SR.DENSE_CASES)
@pytest.mark.parametrize("which", ["r", "c", "rc"])
def test_the_preconditioned_model_reaches_the_dense_solution(name, which):
    """the bound is kappa(N) tol on the relative error of the full x, kappa(N) <= 100 from the dense matrix"""
    c, elim = SR.case(name)
    rng = np.random.default_rng(7)
    r = rng.uniform(-1, 1, (c["m"], 2)) if "r" in which else None
    cv = rng.uniform(-1, 1, (c["n"], 2)) if "c" in which else None
    mdl, pc = J.model(name, np.float64, True)
    xd, Nm = C.dense_solution(c, r=r, cvec=cv, damping_ab=SR.DENSE_DAMPING)
    kappa = np.linalg.cond(Nm)
    assert kappa <= 100, kappa
    x, st = mdl.solve(r=r, c=cv, precond=pc.apply, tol=TOL, max_steps=200)
    plain = mdl.solve(r=r, c=cv, precond=None, tol=TOL, max_steps=200)[1]
    assert (st["stop"] == 1).all() and pc.status.tolist() == [-1, 0]
    err = np.linalg.norm(x - xd, axis=0) / np.linalg.norm(xd, axis=0)
    print("%s %s: kappa %.1f, iterations %s (unpreconditioned %s), error %s, bound %.1e"
          % (name, which, kappa, st["iterations"], plain["iterations"], err, kappa * TOL))
    assert (err <= kappa * TOL).all(), (err, kappa * TOL)


# ---- the plan builder alone, under the sanitizers -------------------------------------------------------------
def _plan_input(case, elim):
    """the lists of the JacSchurMap that the plan is built from, as the text tools/schur_jacobi_plan_check.cpp reads"""
    t = SR.tables(case, elim)
    sizes = np.ones(case["n"], dtype=np.int64) if case["param_sizes"] is None else np.asarray(case["param_sizes"])
    start = np.concatenate([[0], np.cumsum(sizes)])
    kept = [p for p in range(len(sizes)) if p not in set(elim)]
    widths = sizes[kept]
    arrays = [t["elim_off"], kept, start[kept], widths, np.concatenate([[0], np.cumsum(widths)]),
              np.repeat(np.arange(len(kept)), widths)] + list(t["rows_kept"][:3]) + list(t["rows_elim"][:3])
    words = [case["m"], len(elim)]
    for a in arrays:
        words += [len(a)] + [int(x) for x in a]
    return " ".join(map(str, words))


def test_the_plan_builder_runs_clean_under_the_sanitizers(tmp_path):
    """the builder and a main of its own (tools/schur_jacobi_plan_check.cpp), compiled for the host with
    -fsanitize=address,undefined: no report on the edges case and the hub case, the tables those of the restatement,
    and the refusal of a wide kept param by name"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(B.__file__)))
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "schur_jacobi_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the program carries its runtimes)
                           "-I", os.path.join(root, "baspacho_amd", "csrc"),
                           os.path.join(root, "tools", "schur_jacobi_plan_check.cpp"),
                           os.path.join(root, "baspacho_amd", "csrc", "jac_schur_jacobi.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("edges", "hub"):
        c, elim = J.case(name)
        run = subprocess.run([exe], input=_plan_input(c, list(elim)), capture_output=True, text=True, env=env)
        assert run.returncode == 0 and run.stderr == "", (name, run.returncode, run.stderr[-2000:])
        want, seen = J.plan(name), set()
        for line in run.stdout.splitlines():
            key, count, *vals = line.split()
            assert int(count) == len(vals) and np.array_equal(np.asarray(vals, dtype=np.int64), want[key]), (name, key)
            seen.add(key)
        assert seen == set(TABLES) - {"block_width"}
    wide = {"rows": np.array([0, 1]), "cols": np.array([0, 40]), "m": 2, "n": 42, "param_sizes": [8, 33, 1]}
    run = subprocess.run([exe], input=_plan_input(wide, [0]), capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == ""
    assert run.stdout.strip() == "refused: jacobian schur: kept param 1 has 33 scalars; schur_jacobi takes params of at most 32"
