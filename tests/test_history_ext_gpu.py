"""GPU: the results of the entry maps (Assembly, NormalEquations, SymProduct), of the factor products and of the
BAL DevicePipeline do not depend on what the object, or its Solver, was asked to do before
(tests/history_ext.py).

Random walks over the extended vocabulary (seeds committed in history_ext.EXT_WALK_SEEDS, their coverage asserted
on the host by tests/test_history_ext_cpu.py) keep one map per kind alive on a long-lived Solver beside every
operation of tests/history.py; fixed scenarios reach each piece of state a map keeps or borrows: the device
tables uploaded by the first call that needs them, the tables of two maps of one kind, the Solver's pointer ring
and stream, and a call that was refused.  Every result is bitwise the numpy restatement of its owning test
(the factor products: inside the element-wise bound of factor_product_ref), batch members are bitwise their
single calls, and a veteran's bits are a fresh object's.

The DevicePipeline runs LM iterations on one veteran pipeline while a fresh pipeline on a fresh Solver repeats
each iteration from the veteran's parameters: the per-observation buffers, rho, the costs, the ordered H and g in
both precisions and the new parameters must be the same bits, and each stage is held to the reference and bound
of its owning test.

HISTORY_EXT_REPORT=<path>: the worst error / tolerance per family, dtype and metric, as JSON at exit.

Nothing here makes a kernel spin, time out or fault: the refusals are argument checks of the Python layer."""
import atexit
import gc
import json
import os

import numpy as np
import pytest
import torch

import history as H
import history_ext as X
import kf_structures as K
from assembly_ref import stored_elements
from buffer_edges import Frame, is_sentinel
from helpers import solver_random
from history import F32, F64
from history_ext import same_bits

pytestmark = pytest.mark.gpu

S = H.STRUCTURES
REPORT = {}
_REPORT_PATH = os.environ.get("HISTORY_EXT_REPORT")
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
KINDS = list(X.NEW_FAMILIES)
OP_OF = {op.family: op.name for op in X.EXT_OPS if not op.control}


@atexit.register
def _write_report():
    if _REPORT_PATH and REPORT:
        with open(_REPORT_PATH, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _host(outs):
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _full(kind):
    """the variant with the most to go wrong: triangle "full" (skipped entries) where the kind has one"""
    return X.VARIANTS[kind][-1]


def _all_calls(c, m, i, order=None):
    """{call: host outputs per member} of every call of the case, in `order`, each checked against its
    restatement"""
    got = {}
    for call in (c.calls if order is None else order):
        got[call] = _host(c.run(m, call, i)[0])
        c.check(call, i, got[call])
    return got


def _same(a, b, what):
    assert set(a) == set(b)
    for call in a:
        assert len(a[call]) == len(b[call])
        for q, (x, y) in enumerate(zip(a[call], b[call])):
            assert same_bits(x, y), (what, call, "member %d" % q)


# ---- random walks --------------------------------------------------------------------------------------------

WALKS = [(name, seed) for name, seeds in X.EXT_WALK_SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("name,seed", WALKS, ids=["%s-%d" % w for w in WALKS])
def test_random_walk(name, seed):
    steps = H.random_history(seed, X.EXT_WALK_LENGTH, X.EXT_VOCABULARY)
    print("\n".join(H.describe(steps)))
    report = {}
    sol = H.run_history(S[name], steps, tag="ext-walk/%s/%d" % (name, seed), report=report)
    sol.setStream(None)
    for fam, r in report.items():
        if fam in X.NEW_FAMILIES:
            print("worst error / tolerance", fam, json.dumps(r, sort_keys=True))
        for who, per in r.items():
            for dt, metrics in per.items():
                d = REPORT.setdefault(fam, {}).setdefault(who, {}).setdefault(dt, {})
                for k, v in metrics.items():
                    d[k] = max(d.get(k, 0.0), v)
    c = sol.runCounters()
    assert c["sweep_timeouts"] == 0 and c["sweep_error_pending"] == 0, c


# ---- first-use order -----------------------------------------------------------------------------------------

FIRST = [(kind, call) for kind in KINDS for call in X.CASES[kind].calls]
_NATURAL = {}


def _sequence(structure, c, i, order):
    """every call in `order` on a new map of a new Solver"""
    sol = structure()
    return _all_calls(c, c.make(sol), i, order)


@DTYPES
@pytest.mark.parametrize("kind,first", FIRST, ids=["%s-%s" % f for f in FIRST])
def test_first_use_order(kind, first, dtype):
    """the first call on a new map is `first`, then all the others: each part of the map is uploaded (the plan
    of the factor products built) by whichever call comes first; bitwise the restatement, and bitwise a map whose
    first call was the natural one (assemble, hessian, mv, mulL)"""
    st = S["widths"]
    c = X.case(st, kind, _full(kind))
    i = st.cached(("first-use inputs", kind, dtype), lambda: c.inputs(dtype, 41, batch=2, q=3))
    if (kind, dtype) not in _NATURAL:
        _NATURAL[kind, dtype] = _sequence(st, c, i, c.calls)
    got = _sequence(st, c, i, [first] + [x for x in c.calls if x != first])
    _same(got, _NATURAL[kind, dtype], "first call %s" % first)


# ---- precision alternation -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_precision_alternation_on_one_map(kind):
    """f32, f64, f32 through every call of one map: each bitwise a fresh map of that precision"""
    st = S["bipartite"]
    c = X.case(st, kind, _full(kind))
    sol = st()
    m = c.make(sol)
    for k, dtype in enumerate((F32, F64, F32)):
        i = c.inputs(dtype, 50 + k, batch=(1, 2, 5)[k], q=(17, 1, 3)[k])
        _same(_all_calls(c, m, i), _sequence(st, c, i, c.calls), "precision step %d (%s)" % (k, dtype.name))


# ---- two maps of one kind on one Solver ----------------------------------------------------------------------

def _permuted(c0, seed):
    """the case of c0's entry list in another order: tables of the same sizes with other contents"""
    p = np.random.default_rng(seed).permutation(len(c0.rows))
    lists = (c0.rows[p], c0.cols[p]) + ((c0.m,) if c0.kind == "normal_eq" else ())
    return type(c0)(c0.S, c0.variant, lists=lists)


@DTYPES
@pytest.mark.parametrize("kind", X.MAP_KINDS)
def test_two_maps_of_one_kind_then_a_third(kind, dtype):
    """two maps with different entry lists on one Solver, called alternately; one is destroyed and a third, with
    yet another list, is created (where the destroyed one lay, if the allocator reuses the block) and called:
    every result is bitwise its own restatement.  The lists are permutations of one list: every table of one map
    is as large as its twin in the other, so nothing but the contents tells the maps apart"""
    st = S["widths"]
    a = X.case(st, kind, _full(kind))
    b, c3 = _permuted(a, 1), _permuted(a, 2)
    assert not np.array_equal(a.rows, b.rows) and not np.array_equal(b.rows, c3.rows)
    sol = st()
    ma, mb = a.make(sol), b.make(sol)
    ia, ib, ic = (c.inputs(dtype, 60 + k, batch=2, q=3) for k, c in enumerate((a, b, c3)))
    for rnd in range(2):
        for call in a.calls:  # (alternately: every table of both maps is uploaded between calls of the other)
            a.check(call, ia, _host(a.run(ma, call, ia)[0]))
            b.check(call, ib, _host(b.run(mb, call, ib)[0]))
    del mb
    gc.collect()
    mc = c3.make(sol)
    _all_calls(c3, mc, ic)
    _all_calls(a, ma, ia)
    _all_calls(c3, mc, ic, order=c3.calls[::-1])


# ---- the Solver's stream and history -------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("kind", KINDS)
def test_stream_and_history_of_the_solver(kind, dtype):
    """a veteran Solver that has factored a batch of 17 and run selected inversion makes a map and calls it; the
    Solver is given a second stream (handed over through an event) and the map, made before, is called after;
    then on the default stream again.  Veteran and fresh agree bitwise at every step (run_history)"""
    name = OP_OF[kind]
    steps = X.ext_steps(("factor", dtype, 17, 1, 71), ("selectedInverse+marginals", dtype, 1, 1, 72),
                        (name, dtype, 5, 3, 73), ("setStream=second", dtype, 1, 1, 1), (name, dtype, 2, 17, 74),
                        (name, dtype, 1, 1, 75), ("setStream=default", dtype, 1, 1, 1), (name, dtype, 2, 8, 76))
    sol = H.run_history(S["bipartite"], steps, tag="stream/%s/%s" % (kind, dtype.name), report=REPORT)
    sol.setStream(None)
    assert kind == "factor_product" or len(X.maps_of(sol)) >= 1


# ---- shrinking batches ---------------------------------------------------------------------------------------

def _members_are_single_calls(c, m, i, members=None, what=""):
    """every call on the batch of `i`; the members named (all by default) bitwise their single calls and their
    restatements"""
    for call in c.calls:
        outs = c.run(m, call, i)[0]
        torch.cuda.synchronize()
        for b in (range(i["batch"]) if members is None else members):
            got = outs[b].cpu().numpy()
            one = _host(c.run(m, call, i, sel=b)[0])
            assert same_bits(got, one[0]), (what, call, "member %d of %d is not its single call" % (b, i["batch"]))
            c.check(call, i, [got], sel=b)


@DTYPES
@pytest.mark.parametrize("kind", KINDS)
def test_shrinking_batches(kind, dtype):
    """batches of 17, 1, 5 and a single call on one map (on one Solver for mulL / mulLt), every member with
    values of its own: the staged pointers of the larger batch lie behind those of the smaller one"""
    st = S["widths"]
    c = X.case(st, kind, _full(kind))
    sol = st()
    m = c.make(sol)
    for k, batch in enumerate((17, 1, 5, 1)):
        i = c.inputs(dtype, 80 + k, batch=batch, q=(3, 17, 1, 2)[k], members=batch)
        _members_are_single_calls(c, m, i, what="batch %d" % batch)


def _tiny_structure():
    """the solver of test_batch_past_chunk_limit (tests/test_assembly_gpu.py)"""
    return H.Structure("tiny", lambda: solver_random(74, size=4, fill=0.5, pmin=1, pmax=2)[0])


def _stored_cases(st):
    """{kind: case} on the stored elements of a small structure: one entry per element; one Jacobian row per
    element (i, j) holding the columns i and j"""
    r, c = stored_elements(st.host)
    jr = np.concatenate([np.arange(len(r)), np.arange(len(r))[r != c]])
    jc = np.concatenate([r, c[r != c]])
    return {"assembly": X.AssemblyCase(st, "lower", lists=(r, c)), "sym_product": X.SymProductCase(st, "lower", lists=(r, c)),
            "normal_eq": X.NormalEqCase(st, None, lists=(jr, jc, len(r))), "factor_product": X.FactorProductCase(st)}


CHUNK_BATCH = {"assembly": 70000, "normal_eq": 65537, "sym_product": 65537, "factor_product": 65537}


@pytest.mark.parametrize("kind", KINDS)
def test_batch_past_the_chunk_limit_then_a_batch_of_two(kind):
    """a batch that is split into chunks of 65535 members (the batch sizes of test_batch_past_chunk_limit), then
    a batch of 2 on the same map: the members around the chunk boundary and both members of the small batch are
    bitwise their single calls"""
    st = _tiny_structure()
    c = _stored_cases(st)[kind]
    sol = st()
    m = c.make(sol)
    batch = CHUNK_BATCH[kind]
    kw = {"provided": False} if kind == "factor_product" else {}
    big = c.inputs(F32, 90, batch=batch, q=1, **kw)
    _members_are_single_calls(c, m, big, members=(0, 65534, 65535, batch - 1), what="past the chunk limit")
    small = c.inputs(F32, 91, batch=2, q=1, members=2, **kw)
    _members_are_single_calls(c, m, small, what="batch of 2 after %d" % batch)


# ---- the pointer ring ----------------------------------------------------------------------------------------

@DTYPES
def test_ring_wrap(dtype):
    """40 batched calls of the maps and of mulL / mulLt, each followed by a batched solveLt, queued on one Solver
    with no host synchronisation in between: the ring of 32 pointer slots wraps more than twice, and a slot is
    rewritten only after its call's kernels.  Afterwards every result is bitwise the same call made alone"""
    st = H.Structure("tiny24", lambda: K.dense_solver(24, span=3))
    cases = _stored_cases(st)
    sol = st()
    maps = {kind: c.make(sol) for kind, c in cases.items()}
    n, nrhs = sol.order(), 3
    L = st.provided("kf", 3, dtype)
    plan = []
    for k in range(40):
        kind = KINDS[k % len(KINDS)]
        c = cases[kind]
        call = c.calls[(k // len(KINDS)) % len(c.calls)]
        i = c.inputs(dtype, 1000 + k, batch=2 + k % 3, q=1 + k % 2, members=2 + k % 3)
        rhs = [np.random.default_rng(2000 + 10 * k + q).standard_normal((nrhs, n)).astype(dtype) for q in range(2 + k % 3)]
        plan.append({"kind": kind, "call": call, "i": i, "st": c.stage(call, i), "rhs": rhs,
                     "mats": [H._dev(L) for _ in rhs], "vecs": [H._dev(r) for r in rhs]})
    for kind, c in cases.items():  # the tables are uploaded (a host copy that waits) before the queue is built
        _all_calls(c, maps[kind], c.inputs(dtype, 5, batch=2, q=2))
    sol.solveLt([H._dev(L), H._dev(L)], [H._dev(plan[0]["rhs"][0]), H._dev(plan[0]["rhs"][1])], n, nrhs)
    torch.cuda.synchronize()
    outs = []
    for p in plan:
        outs.append(cases[p["kind"]].launch(maps[p["kind"]], p["st"]))
        sol.solveLt(p["mats"], p["vecs"], n, nrhs)
    assert sol._testPtrRingSlotBytes() == 512  # 64 pointers: never grown, so the 32 slots wrapped
    torch.cuda.synchronize()
    for k, (p, o) in enumerate(zip(plan, outs)):
        c, m, i = cases[p["kind"]], maps[p["kind"]], p["i"]
        got = [t.cpu().numpy() for t in o]
        c.check(p["call"], i, got)
        for b in range(i["batch"]):
            one = _host(c.run(m, p["call"], i, sel=b)[0])
            assert same_bits(got[b], one[0]), ("queued call %d" % k, p["kind"], p["call"], "member %d" % b)
            v = H._dev(p["rhs"][b])
            sol.solveLt(H._dev(L), v, n, nrhs)
            assert same_bits(p["vecs"][b].cpu().numpy(), v.cpu().numpy()), ("queued solveLt %d" % k, b)


# ---- after a refusal -----------------------------------------------------------------------------------------

def _refusals(kind, m, dev, out):
    """[(what, exception, call)]: a wrong last dimension, a wrong dtype pairing, an `out` of the wrong shape"""
    other = torch.float32 if out.dtype == torch.float64 else torch.float64
    if kind == "assembly":
        (v,) = dev
        return [("last dimension", ValueError, lambda: m.assemble(v[:-1], out=out)),
                ("dtype pairing", ValueError, lambda: m.assemble(v.to(other), out=out)),
                ("shape of out", ValueError, lambda: m.assemble(v, out=out[:-1]))]
    if kind == "normal_eq":
        v, r = dev
        return [("last dimension", ValueError, lambda: m.jtVec(v[:-1], r, out=out)),
                ("dtype pairing", TypeError, lambda: m.jtVec(v, r.to(other), out=out)),
                ("shape of out", ValueError, lambda: m.jtVec(v, r, out=out[:, :1]))]
    v, x = dev
    return [("last dimension", ValueError, lambda: m.mv(v[:-1], x, out=out)),
            ("dtype pairing", TypeError, lambda: m.mv(v, x.to(other), out=out)),
            ("shape of out", ValueError, lambda: m.mv(v, x, out=out[:, :1]))]


@DTYPES
@pytest.mark.parametrize("kind", X.MAP_KINDS)
def test_after_a_refusal(kind, dtype):
    """each refused call raises and writes nothing (the output lies in a frame of sentinels); the next valid call
    on the same map, into the same output, is bitwise the restatement"""
    st = S["widths"]
    c = X.case(st, kind, _full(kind))
    call = {"assembly": "assemble", "normal_eq": "jtVec", "sym_product": "mv"}[kind]
    sol = st()
    m = c.make(sol)
    i = c.inputs(dtype, 95, batch=1, q=2)
    _all_calls(c, m, i)
    stg = c.stage(call, i)
    shape = tuple(stg["out"].shape)
    for k in range(3):
        fr = Frame([int(np.prod(shape))], dtype)
        out = fr.view(0).view(shape)
        what, exc, refused = _refusals(kind, m, stg["dev"], out)[k]
        with pytest.raises(exc):
            refused()
        torch.cuda.synchronize()
        fr.assert_intact(what=what)
        assert is_sentinel(fr.host(0)).all(), (what, "a refused call wrote to out")
        stg["out"] = out
        got = _host(c.launch(m, stg))
        fr.assert_intact(what="the valid call after: " + what)
        c.check(call, i, got)
    _all_calls(c, m, i)


# ---- the BAL DevicePipeline ----------------------------------------------------------------------------------

LOSS_A = 2.0          # the loss size of tests/test_bal_step_gpu.py
LAM = 1e-3
PIPE_BITWISE = ("res_lin", "Jc_lin", "Jp_lin", "res", "Jc", "Jp", "rho", "cost_linearized", "H64", "g64", "H32", "g32",
                "cand_res", "cand_rho", "cand_cost", "cams", "pts")
_PIPE = {}


def _pipe_scene(cam_size):
    """4 cameras and 131 points: camera 0 sees every point (131 observations: two chunks of the ordered fill's
    128), camera 1 the points 0 .. 69, camera 2 the points 60 .. 130, camera 3 every third; every point is seen
    by two cameras at least; a tenth of the observations are gross outliers.  (problem, solver factory, layout)"""
    import baspacho_amd as B
    import bal_ref as R
    from baspacho_amd import bal
    if "prob" not in _PIPE:
        sees = [np.arange(131), np.arange(70), np.arange(60, 131), np.arange(0, 131, 3)]
        oc = np.concatenate([np.full(len(s), k) for k, s in enumerate(sees)])
        order = np.random.default_rng(5).permutation(len(oc))
        p = bal.synth_scene_for(4, 131, oc[order], np.concatenate(sees)[order], seed=7)
        rng = np.random.default_rng(6)   # (one observation in ten off by 40 .. 80 px: the robust losses keep work)
        bad = rng.choice(len(oc), len(oc) // 10, replace=False)
        xy = p.obs_xy.copy()
        xy[bad] += rng.choice([-1.0, 1.0], (len(bad), 2)) * rng.uniform(40, 80, (len(bad), 2))
        _PIPE["prob"] = bal.BalProblem(p.cams, p.pts, p.obs_cam, p.obs_pt, xy)
    prob = _PIPE["prob"]
    if cam_size not in _PIPE:
        sizes, ss, ranges = bal.bal_structure(prob, cam_size=cam_size)
        make = lambda: B.create_solver(B.Settings(), sizes, ss, ranges)  # noqa: E731
        _PIPE[cam_size] = (make, R.layout(make(), prob.num_pts, prob.num_cams, cam_size))
    return (prob,) + _PIPE[cam_size]


def _np(t):
    return t.detach().cpu().numpy().copy()


def _residual_error(param, prob, cams, pts, res):
    """the worst residual error against mpmath in the scale of bal_ref.lin_errors: |projection| + |xy|"""
    import bal_ref as R
    mp = R._mp()
    worst = 0.0
    res = np.asarray(res).reshape(-1, 2)
    with mp.workdps(R.DPS):
        zero6, zero3 = [mp.mpf(0)] * 6, [mp.mpf(0)] * 3
        f = lambda a: [mp.mpf(float(v)) for v in a]  # noqa: E731
        for o, (c, p, xy) in enumerate(zip(prob.obs_cam, prob.obs_pt, prob.obs_xy)):
            xym = f(xy)
            r = R.residual_bal9(f(cams[c]), f(pts[p]), xym) if param == "bal9" else \
                R.residual_se3(f(cams[c]), f(pts[p]), xym, zero6, zero3)
            scale = max(abs(r[0] + xym[0]), abs(r[1] + xym[1])) + max(abs(xym[0]), abs(xym[1]))
            e = max(abs(mp.mpf(float(res[o, 0])) - r[0]), abs(mp.mpf(float(res[o, 1])) - r[1])) / scale
            worst = max(worst, float(e))
    return worst


def _loss_name(loss):
    return "trivial" if loss is None else loss[0]


def _set_loss(pipe, loss):
    from baspacho_amd import bal
    pipe.loss_kind, pipe.loss_a = (0, 1.0) if loss is None else (bal.LOSS_KINDS[loss[0]], float(loss[1]))


def _expected(prob, cs, lay, Jc, Jp, res, dtype):
    import bal_fill_ref as F
    return F.blockwise_expected(prob.num_pts, prob.num_cams, cs, prob.obs_cam, prob.obs_pt, Jc, Jp, res, lay, dtype)


def _iteration(pipe, prob, lay, priors=None, step=None):
    """one LM iteration on `pipe`: linearize, apply_loss, cost_linearized, the atomic fill, the ordered fill in
    fp64 then fp32 (onto `priors`, drawn here when None), factor + solve, apply_step (of `step` when given: the
    atomics of the factor then stay out of the comparison), cost(candidate), set_params.  -> host arrays"""
    import bal_ref as R
    sol, cs, n = pipe.solver, pipe.cam_size, pipe.solver.order()
    out = {"cams_in": _np(pipe.cams).reshape(-1, 9), "pts_in": _np(pipe.pts).reshape(-1, 3)}
    pipe.linearize()
    out.update(res_lin=_np(pipe.res), Jc_lin=_np(pipe.Jc), Jp_lin=_np(pipe.Jp))
    pipe.apply_loss()
    out.update(res=_np(pipe.res), Jc=_np(pipe.Jc), Jp=_np(pipe.Jp), rho=_np(pipe.rho))
    out["cost_linearized"] = _np(pipe.cost_linearized()).reshape(1)
    if priors is None:
        priors = {}
        for dtype in (np.float64, np.float32):
            exp = _expected(prob, cs, lay, out["Jc"], out["Jp"], out["res"], dtype)
            priors[dtype] = (exp, R.prior_for(exp, dtype, seed=len(out["res"]) + cs))
    out["priors"] = priors
    Ha = torch.zeros(sol.dataSize(), dtype=torch.float64, device="cuda")
    ga = torch.zeros(n, dtype=torch.float64, device="cuda")
    pipe.fill_hessian(Ha, ga, LAM)
    out.update(Ha=_np(Ha), ga=_np(ga))
    for dtype, tag in ((np.float64, "64"), (np.float32, "32")):
        Hd, gd = (H._dev(p) for p in priors[dtype][1])
        pipe.fill_hessian_ordered(Hd, gd, LAM)
        out["H" + tag], out["g" + tag] = _np(Hd), _np(gd)
    mine = ga.clone()
    sol.factor(Ha)
    sol.solve(Ha, mine, n, 1)
    out["step"] = _np(mine)
    cams, pts = pipe.apply_step(mine if step is None else H._dev(step))
    out["cand_cost"] = _np(pipe.cost(cams, pts)).reshape(1)
    out.update(cand_res=_np(pipe._cand_res), cand_rho=_np(pipe._cand_rho), cams=_np(cams), pts=_np(pts))
    pipe.set_params(cams, pts)
    torch.cuda.synchronize()
    return out


def _check_iteration(param, loss, pipe, prob, lay, o, what):
    """every stage of the iteration `o` against the reference and bound of its owning test"""
    import bal_fill_ref as F
    import bal_ref as R
    import bal_step_ref as SR
    cs, n_obs, kind = pipe.cam_size, len(prob.obs_cam), _loss_name(loss)
    a = 1.0 if loss is None else loss[1]
    # residuals, at the parameters the iteration started from and at the candidate (test_bal_step_gpu.py)
    for res, cams, pts, which in ((o["res_lin"], o["cams_in"], o["pts_in"], "linearize"),
                                  (o["cand_res"], o["cams"].reshape(-1, 9), o["pts"].reshape(-1, 3), "candidate")):
        e = _residual_error(param, prob, cams, pts, res)
        assert e <= R.LIN_BOUND, (what, which, "residual", e)
    # the loss: rho and the scaled words, observations of weight 1 bitwise intact
    pairs = [(o[k + "_lin"].reshape(n_obs, -1), o[k].reshape(n_obs, -1)) for k in ("res", "Jc", "Jp")]
    e_rho, e_w = SR.loss_errors(kind, a, o["res_lin"], o["rho"], pairs)
    assert e_rho <= SR.LOSS_BOUND and e_w <= SR.LOSS_BOUND, (what, "loss", e_rho, e_w)
    unit = SR.unit_weight(kind, a, o["res_lin"])
    for before, after in pairs:
        assert same_bits(after[unit], before[unit]), (what, "an observation of weight 1 was rewritten")
    e_rho, _ = SR.loss_errors(kind, a, o["cand_res"], o["cand_rho"], [])
    assert e_rho <= SR.LOSS_BOUND, (what, "candidate rho", e_rho)
    # the sums: bitwise the documented order
    assert same_bits(o["cost_linearized"], np.array([SR.sum_model(o["rho"], 0.5)])), (what, "cost_linearized")
    assert same_bits(o["cand_cost"], np.array([SR.sum_model(o["cand_rho"], 0.5)])), (what, "cost(candidate)")
    # the fills: the atomic one at its bound (bal_ref), the ordered one at that bound and bitwise its model
    tab = pipe.fill_plan()._testTables()
    inputs = (o["Jc"].reshape(n_obs, 2, cs), o["Jp"].reshape(n_obs, 2, 3), o["res"].reshape(n_obs, 2))
    exp64 = o["priors"][np.float64][0]
    zero = [np.zeros(len(o["Ha"])), np.zeros(len(o["ga"]))]
    F.check_fill(lay["diag"], np.float64, exp64, zero, o["Ha"], o["ga"], LAM, (what, "atomic fill"))
    for dtype, tag in ((np.float64, "64"), (np.float32, "32")):
        exp, prior = o["priors"][dtype]
        F.check_fill(lay["diag"], dtype, exp, prior, o["H" + tag], o["g" + tag], LAM, (what, "ordered fill", tag))
        want, wantg = F.model_fill(tab, *inputs, prior, dtype, LAM, lay["diag"])
        assert same_bits(o["H" + tag], want) and same_bits(o["g" + tag], wantg), (what, "ordered fill vs model", tag)
    return tab


def _check_retraction(param, pipe, prob, o, step, what):
    import bal_step_ref as SR
    sol, cs, npt, nc = pipe.solver, pipe.cam_size, prob.num_pts, prob.num_cams
    perm = sol.paramToSpan()
    off = np.array([sol.spanVectorOffset(int(perm[p])) for p in range(npt + nc)], dtype=np.int64)
    cams, pts = o["cams"].reshape(nc, 9), o["pts"].reshape(npt, 3)
    assert same_bits(pts, o["pts_in"] - step[off[:npt, None] + np.arange(3)]), (what, "points")
    cam_step = step[off[npt:, None] + np.arange(cs)]
    if param == "bal9":
        assert same_bits(cams, o["cams_in"] - cam_step), (what, "cameras")
    else:
        eR, eT = SR.step_errors(o["cams_in"], cam_step, cams)
        assert eR.max() <= SR.STEP_BOUND_R and eT.max() <= SR.STEP_BOUND_T, (what, eR.max(), eT.max())
        assert same_bits(cams[:, 6:9], o["cams_in"][:, 6:9]), (what, "the calibration is copied")


LOSSES = [None, ("huber", LOSS_A), ("cauchy", LOSS_A)]


@pytest.mark.parametrize("loss", LOSSES, ids=["trivial", "huber", "cauchy"])
@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_pipeline_veteran_against_fresh(param, loss):
    """three LM iterations on one veteran pipeline (its loss switched between them: the parametrised one, the
    other kind -- trivial for a robust loss, Huber for the trivial one -- and the first again), each repeated by
    a fresh pipeline on a fresh Solver from the veteran's parameters and step: same bits in every
    per-observation buffer, rho, the costs, the ordered H and g in both precisions and the new parameters"""
    from baspacho_amd import bal
    cs = 9 if param == "bal9" else 6
    prob, make, lay = _pipe_scene(cs)
    veteran = bal.DevicePipeline(prob, make(), param=param, loss=loss)
    assert veteran.fill_plan().info()["max_cam_list"] > veteran.fill_plan().info()["C"] == 128
    other = ("huber", LOSS_A) if loss is None else None
    for k, now in enumerate((loss, other, loss)):
        what = "%s/%s iteration %d (%s)" % (param, _loss_name(loss), k, _loss_name(now))
        _set_loss(veteran, now)
        at = bal.BalProblem(_np(veteran.cams).reshape(-1, 9), _np(veteran.pts).reshape(-1, 3), prob.obs_cam,
                            prob.obs_pt, prob.obs_xy)
        v = _iteration(veteran, prob, lay)
        assert all(np.isfinite(v[key]).all() for key in PIPE_BITWISE + ("step",)), what
        _check_iteration(param, now, veteran, prob, lay, v, what)
        _check_retraction(param, veteran, prob, v, v["step"], what)
        fresh = bal.DevicePipeline(at, make(), param=param, loss=now)
        f = _iteration(fresh, prob, lay, priors=v["priors"], step=v["step"])
        for key in PIPE_BITWISE:
            assert same_bits(v[key], f[key]), (what, "the veteran's %s is not bitwise the fresh pipeline's" % key)
        if now is not None:
            assert not same_bits(v["res"], v["res_lin"]), (what, "the robust loss scaled nothing")
    print(param, _loss_name(loss), "costs", [float(v["cost_linearized"][0]), float(v["cand_cost"][0])])


@DTYPES
@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_two_pipelines_with_two_fill_plans_on_one_solver(param, dtype):
    """two pipelines on one Solver whose observation lists hold the same (camera, point) pairs in another order,
    one of them with seven observations a second time: two BalFillPlans, called alternately; each ordered fill
    is bitwise the model of its own plan and inside the bound of its own reference"""
    import bal_fill_ref as F
    import bal_ref as R
    from baspacho_amd import bal
    cs = 9 if param == "bal9" else 6
    prob, make, lay = _pipe_scene(cs)
    sol = make()
    rng = np.random.default_rng(3)
    order = np.concatenate([rng.permutation(len(prob.obs_cam)), rng.choice(len(prob.obs_cam), 7, replace=False)])
    xy = prob.obs_xy[order].copy()
    xy[-7:] += np.linspace(-3, 3, 14).reshape(7, 2)
    second = bal.BalProblem(prob.cams, prob.pts, prob.obs_cam[order], prob.obs_pt[order], xy)
    pipes = [(bal.DevicePipeline(p, sol, param=param), p) for p in (prob, second)]
    tabs = [pipe.fill_plan()._testTables() for pipe, _ in pipes]
    assert pipes[0][0].fill_plan() is not pipes[1][0].fill_plan() and tabs[1]["kept"] == tabs[0]["kept"] + 7
    assert not np.array_equal(tabs[0]["camObs"], tabs[1]["camObs"][:len(tabs[0]["camObs"])])
    seen = []
    for rnd in range(2):
        for pipe, _ in pipes:
            pipe.linearize()
        for k, (pipe, p) in enumerate(pipes):
            n_obs = len(p.obs_cam)
            inputs = (_np(pipe.Jc).reshape(n_obs, 2, cs), _np(pipe.Jp).reshape(n_obs, 2, 3), _np(pipe.res).reshape(n_obs, 2))
            exp = _expected(p, cs, lay, *inputs, dtype)
            prior = R.prior_for(exp, dtype, seed=11 + k)
            Hd, gd = (H._dev(a) for a in prior)
            pipe.fill_hessian_ordered(Hd, gd, LAM)
            got, gotg = _np(Hd), _np(gd)
            F.check_fill(lay["diag"], dtype, exp, prior, got, gotg, LAM, (param, "pipeline %d" % k, "round %d" % rnd))
            want, wantg = F.model_fill(tabs[k], *inputs, prior, dtype, LAM, lay["diag"])
            assert same_bits(got, want) and same_bits(gotg, wantg), (param, "pipeline %d" % k, "round %d" % rnd)
            seen.append((got, gotg))
    for k in range(2):  # the second round, after the other pipeline's fill, gives the bits of the first
        assert same_bits(seen[k][0], seen[k + 2][0]) and same_bits(seen[k][1], seen[k + 2][1])
