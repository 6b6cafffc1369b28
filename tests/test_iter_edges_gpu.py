"""GPU: the pieces of the conjugate gradient and of the Lanczos recurrence (bsp_cg_*, bsp_lanczos_*; DESIGN.md
sections 24 and 25) and the batched error-bound calls on framed, poisoned and exact-size buffers (DESIGN.md
section 5, "Buffer edges").

tests/iter_driver.py issues the piece sequence of CgRun.run / LanczosRun.run on buffers that are all the
test's: every vector operand of every member is a payload of a buffer_edges.Frame (sentinel NaNs all round, odd
element offsets), the members of a batch of 2 lie in different frames in descending address order, the records
and coefficients lie in a float64 frame, and the work areas are 16-byte-aligned payloads of exactly
bsp_*_work_bytes x batch bytes.  Everything a run writes before it reads starts as the sentinel, not as zero:
p, Ap, z, minv, the records, the status and the work of CG; the whole basis with the gaps between its slots
(slot_stride = n q + 5), w, the coefficients, the records and the work of Lanczos.

After EVERY piece: Frame.assert_intact with the complement of the piece's declared write set
(iter_driver.WRITE_SETS) as the read-only set, and, for the operands the piece may write, the columns of
stopped problems, the other basis slots and the coefficient entries of other steps bitwise what they were.  At
the end x, the records, the preconditioner's status, alpha, beta and the basis are bitwise the numpy
restatements (cg_ref.entries_model, lanczos_ref.entries_model), and whatever no step wrote still holds the
sentinel.  No tolerance enters: every comparison is of bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cg_ref as R
import error_bounds_ref as E
import iter_driver as D
import lanczos_ref as LR
from buffer_edges import Frame, SENTINEL_BITS, framed, is_sentinel
from test_cg_gpu import _tri_case
from test_error_bounds_gpu import _factor, _pattern_of

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64, 1e-8), "f32": (torch.float32, np.float32, 1e-4)}
GUARD = 256
STEPS = 6      # CG iterations
KMAX = 10      # Lanczos steps: the projection counts 1 .. 10 cross the group of 8
PAD = 5        # slot_stride = n q + PAD
P, I32, I64, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
KIND_NAME = {None: None, 0: "given", 1: "jacobi", 2: "block_jacobi"}
POISON64 = np.int64(SENTINEL_BITS[np.float64])


def _words(a):
    """host array as integer words"""
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dense(n, rows, cols, v):
    A = np.zeros((n, n))
    np.add.at(A, (rows, cols), v)
    return A + np.tril(A, -1).T


def _half(r):
    """the caller's preconditioner of kind 0: z = r / 2, exact in both precisions"""
    return (r * r.dtype.type(0.5)).astype(r.dtype)


# ---- the buffers of a run ------------------------------------------------------------------------------------
class Buffers:
    """the frames of one run and the check after every piece.  member: names of the per-member operands in the
    member frames' payload order, shared: names of the float64-word operands that hold all members one after the
    other; aligned: names of the exact-size 16-byte-aligned work areas (sizes in bytes)"""

    def __init__(self, npdt, nb, member_sizes, shared_sizes, aligned_bytes):
        self.npdt, self.nb = np.dtype(npdt), nb
        self.member_names = list(member_sizes)
        frames = [Frame(list(member_sizes.values()), npdt, guard=GUARD) for _ in range(nb)]
        frames.sort(key=lambda f: -f.base.data_ptr())       # member 0 at the highest address
        assert all(frames[m].base.data_ptr() > frames[m + 1].base.data_ptr() for m in range(nb - 1))
        self.members = frames
        self.shared_names = list(shared_sizes)
        self.shared = Frame(list(shared_sizes.values()), np.float64, guard=GUARD)
        self.aligned_names = list(aligned_bytes)
        assert all(b % 16 == 0 for b in aligned_bytes.values())
        self.aligned = Frame([b // 8 for b in aligned_bytes.values()], np.float64, guard=GUARD, align_bytes=16)
        self.prev = {}

    # -- access
    def op(self, name):
        """the member views of a per-member operand (what the driver is handed)"""
        k = self.member_names.index(name)
        return [f.view(k) for f in self.members]

    def addr(self, name):
        if name in self.shared_names:
            return self.shared.view(self.shared_names.index(name)).data_ptr()
        v = self.aligned.view(self.aligned_names.index(name))
        assert v.data_ptr() % 16 == 0
        return v.data_ptr()

    def fill(self, name, m, a):
        self.members[m].fill(self.member_names.index(name), np.ascontiguousarray(a, dtype=self.npdt))

    def host(self, name, m=None):
        if name in self.member_names:
            return self.members[m].host(self.member_names.index(name))
        return self.shared.host(self.shared_names.index(name))

    def snapshot(self, names):
        out = {}
        for name in names:
            if name in self.member_names:
                out[name] = [self.host(name, m) for m in range(self.nb)]
            else:
                out[name] = self.host(name)
        return out

    def seal(self, watched):
        for f in self.members + [self.shared, self.aligned]:
            f.seal()
        self.prev = self.snapshot(watched)

    def assert_frames(self, writes, what):
        """guards intact everywhere; every payload whose name is not in `writes` bitwise what it was"""
        ro = [k for k, name in enumerate(self.member_names) if name not in writes]
        for m, f in enumerate(self.members):
            f.assert_intact(read_only=ro, what="%s, member %d" % (what, m))
        self.shared.assert_intact(read_only=[k for k, name in enumerate(self.shared_names) if name not in writes],
                                  what=what + ", records")
        self.aligned.assert_intact(read_only=[k for k, name in enumerate(self.aligned_names) if name not in writes],
                                   what=what + ", work")


def _frozen_columns(prev, cur, stopped, q, what):
    """the columns `stopped` (bool [q]) of the [n, q] operand are bitwise what they were"""
    a, b = _words(prev).reshape(-1, q), _words(cur).reshape(-1, q)
    bad = (a != b).any(axis=0) & stopped
    assert not bad.any(), (what, "the columns %s of stopped problems changed" % np.nonzero(bad)[0].tolist())


# ---- the conjugate gradient ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cg_case(n, q, nb, dt, kind):
    """host inputs and the restatement's results per member: a column that runs on, one that converges after an
    iteration or two (b = M v for an eigenvector v of the pencil (A, M), M the preconditioner's matrix), one zero
    right-hand side under a non-zero start"""
    _, npdt, tol = DT[dt]
    rows, cols, values, _, sizes, pat = _tri_case(n)
    prod = R.Product(n, rows, cols)
    bs = np.concatenate([[0], np.cumsum(sizes)])
    out = []
    for m in range(nb):
        rng = np.random.default_rng(1000 * n + 10 * q + m)
        v = values[m].astype(npdt)
        A = _dense(n, rows, cols, v.astype(np.float64))
        if kind == 1:
            M = np.diag(np.diag(A))
        elif kind == 2:
            M = np.zeros_like(A)
            for s0, s1 in zip(bs[:-1], bs[1:]):
                M[s0:s1, s0:s1] = A[s0:s1, s0:s1]
        else:
            M = np.eye(n)
        Lm = np.linalg.cholesky(M)
        G = np.linalg.solve(Lm, np.linalg.solve(Lm, A).T).T      # Lm^-1 A Lm^-T
        u = np.linalg.eigh((G + G.T) / 2)[1][:, n // 2]
        early = M @ np.linalg.solve(Lm.T, u)                     # b = M v, v = Lm^-T u
        early /= np.abs(early).max()
        b = rng.uniform(-1, 1, (n, q))
        x0 = np.zeros((n, q))
        x0[:, 0] = rng.uniform(-0.1, 0.1, n)
        if q == 3:
            b[:, 1], b[:, 2] = early, 0.0
            x0[:, 2] = rng.uniform(-1, 1, n)                     # init must clear it, and r with it
        elif m == 1:
            b[:, 0], x0[:, 0] = early, 0.0
        b, x0 = b.astype(npdt), x0.astype(npdt)
        r0 = (b + (-prod.mv(v, x0, npdt))).astype(npdt)
        precond = _half if kind == 0 else KIND_NAME[kind]
        want_x, st, status = R.entries_model(n, rows, cols, v, b, npdt, precond, param_sizes=sizes, tol=tol,
                                             max_steps=STEPS, x0=x0)
        out.append({"values": v, "b": b, "x0": x0, "r0": r0, "x": want_x, "st": st, "status": status})
    return out


# every value of n, q, batch and precision meets every piece: each preconditioner kind is a piece of its own, so
# each kind gets a trio of shapes that holds every value of every axis
TRIOS = [[(1, 1, 1, "f64"), (255, 3, 2, "f32"), (1025, 3, 2, "f64")],
         [(1, 3, 2, "f32"), (255, 1, 1, "f64"), (1025, 1, 2, "f32")],
         [(1, 1, 2, "f32"), (255, 3, 1, "f64"), (1025, 3, 2, "f32")]]
CG_CASES = [shape + (kind,) for kind, trio in ((None, 1), (0, 2), (1, 2), (2, 0)) for shape in TRIOS[trio]]


def test_the_cg_cases_cover_every_axis_for_every_kind():
    for kind in (None, 0, 1, 2):
        mine = [c for c in CG_CASES if c[4] == kind]
        assert {c[0] for c in mine} == {1, 255, 1025} and {c[1] for c in mine} == {1, 3}, kind
        assert {c[2] for c in mine} == {1, 2} and {c[3] for c in mine} == {"f64", "f32"}, kind


@pytest.mark.parametrize("n,q,nb,dt,kind", CG_CASES,
                         ids=["n%d-q%d-b%d-%s-%s" % (c[0], c[1], c[2], c[3], KIND_NAME[c[4]]) for c in CG_CASES])
def test_cg_pieces_on_framed_poisoned_exact_buffers(n, q, nb, dt, kind):
    tdt, npdt, tol = DT[dt]
    case = _cg_case(n, q, nb, dt, kind)
    rows, cols, _, _, sizes, pat = _tri_case(n)
    sol, prod = pat.solver, pat.product
    nq = n * q
    inv = 1
    if kind in (1, 2):
        info = (ctypes.c_int64 * 4)()
        assert sol._lib.bsp_cg_precond_info(prod._h, I32(kind), info) == 0
        inv = max(int(info[2]), 1)
    W, Wb = D.work_bytes(sol, "cg", n, q), D.work_bytes(sol, "cg", n, 1)
    buf = Buffers(npdt, nb, {"values": len(rows), "b": nq, "x": nq, "r": nq, "p": nq, "ap": nq, "z": nq, "minv": inv},
                  {"state": nb * q * 12, "status": nb * 2}, {"work": W * nb, "build_work": Wb * nb})
    for m, c in enumerate(case):
        for name, key in (("values", "values"), ("b", "b"), ("x", "x0"), ("r", "r0")):
            buf.fill(name, m, c[key])
    watched = ("x", "r", "p", "z", "state")
    buf.seal(watched)
    seen = []

    def hook(piece, step, info):
        torch.cuda.synchronize()
        what = "%s at step %d" % (piece, step)
        writes = D.PRODUCT_WRITES["cg"] if piece == "mv" else D.write_set(piece, kind=info.get("kind"))
        if piece == "cg_precond_build":
            writes = tuple("build_work" if w == "work" else w for w in writes)
        buf.assert_frames(writes, what)
        cur = buf.snapshot(watched)
        was = buf.prev["state"].view(np.int64).reshape(nb, q, 12)
        now = cur["state"].view(np.int64).reshape(nb, q, 12)
        for m in range(nb):
            if piece == "cg_init":
                assert not (now[m] == POISON64).any(), (what, m, "a word of a record was not written")
                zero = now[m, :, 1] == R.ZERO_RHS
                for name in ("x", "r"):
                    _frozen_columns(buf.prev[name][m], cur[name][m], ~zero, q, (what, name, m))
                    assert not cur[name][m].reshape(n, q)[:, zero].any(), (what, name, m, "a zero column is not 0")
            elif piece not in ("cg_precond_build",):
                stopped = was[m, :, 1] != R.RUNNING
                for name in ("x", "r", "p", "z"):
                    _frozen_columns(buf.prev[name][m], cur[name][m], stopped, q, (what, name, m))
                assert (was[m][stopped] == now[m][stopped]).all(), (what, m, "the record of a stopped problem changed")
        buf.seal(watched)
        seen.append(piece)

    def given_z(step):
        for m in range(nb):
            z, r = buf.op("z")[m], buf.op("r")[m]
            z.copy_(r * 0.5)
        buf.seal(watched)

    views = lambda name: [t.view(n, q) for t in buf.op(name)]
    ops = {"values": buf.op("values"), "b": views("b"), "x": views("x"), "r": views("r"), "p": views("p"),
           "ap": views("ap"), "z": None if kind is None else views("z"), "minv": buf.op("minv") if kind in (1, 2) else None}
    run = D.CgPieces(sol, prod, dt, n, q, nb, nb > 1, ops, buf.addr("work"), buf.addr("state"), kind=kind, tol=tol,
                     max_steps=STEPS, build_work=buf.addr("build_work"), status=buf.addr("status"),
                     given_z=given_z if kind == 0 else None, hook=hook)
    run.run()
    want_pieces = {"cg_init", "cg_alpha", "cg_update", "cg_direction", "mv"}
    want_pieces |= set() if kind is None else {"cg_precond"}
    want_pieces |= {"cg_precond_build"} if kind in (1, 2) else set()
    assert set(seen) == want_pieces and seen.count("cg_update") == STEPS

    state = buf.host("state").view(np.int64).reshape(nb, q, 12)
    status = buf.host("status").view(np.int64).reshape(nb, 2)
    its = []
    for m, c in enumerate(case):
        st = c["st"]
        assert _same(buf.host("x", m).reshape(c["x"].shape), c["x"]), (m, "x is not the restatement's")
        for j in range(q):
            np.testing.assert_array_equal(state[m, j], R.record_words(st, j), err_msg="member %d column %d" % (m, j))
        if kind in (1, 2):
            np.testing.assert_array_equal(status[m], c["status"])
        else:
            assert (status[m] == POISON64).all(), "no build ran: the status must still hold the sentinel"
        never = st["stop"] == R.ZERO_RHS                     # p and z of a problem that never started
        for name in ("p",) + (("z",) if kind in (1, 2) else ()):
            got = is_sentinel(buf.host(name, m)).reshape(n, q)
            assert got[:, never].all() and not got[:, ~never].any(), (name, m)
        its += st["iterations"].tolist()
    if n > 1 and (q == 3 or nb == 2):
        assert 0 < min(i for i in its if i > 0) < max(its), ("no problem stopped early beside one that ran on", its)
    if q == 3:
        assert all(c["st"]["stop"][2] == R.ZERO_RHS for c in case)


# ---- the Lanczos recurrence ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lz_case(n, q, nb, dt, reorth):
    _, npdt, _ = DT[dt]
    rows, cols, values, _, _, _ = _tri_case(n)
    out = []
    for m in range(nb):
        rng = np.random.default_rng(2000 * n + 10 * q + m)
        v = values[m].astype(npdt)
        if n >= 8:
            vec = np.linalg.eigh(_dense(n, rows, cols, v.astype(np.float64)))[1]
            early = vec[:, [0, n // 2, n - 1]] @ np.array([1.0, 0.7, -0.6])   # an invariant subspace of dimension 3
        else:
            early = np.ones(n)
        v0 = rng.uniform(-1, 1, (n, q))
        if q == 3:
            v0[:, 1], v0[:, 2] = early, 0.0
        elif m == 1:
            v0[:, 0] = early
        v0 = v0.astype(npdt)
        coef, st, V = LR.entries_model(n, rows, cols, v, v0, npdt, KMAX, reorth=reorth)
        out.append({"values": v, "v0": v0, "coef": coef, "st": st, "V": V})
    return out


LZ_MODES = {"full": ("full", KMAX), "ring": (None, 2), "kept": (None, KMAX)}
LZ_CASES = [shape + (mode,) for mode, trio in (("full", 0), ("ring", 1), ("kept", 2)) for shape in TRIOS[trio]]
LZ_CASES.append((1025, 1, 2, "f32", "full"))


def test_the_lanczos_cases_cover_every_axis_for_every_mode():
    for mode in LZ_MODES:
        mine = [c for c in LZ_CASES if c[4] == mode]
        assert {c[0] for c in mine} == {1, 255, 1025} and {c[1] for c in mine} == {1, 3}, mode
        assert {c[2] for c in mine} == {1, 2} and {c[3] for c in mine} == {"f64", "f32"}, mode


@pytest.mark.parametrize("n,q,nb,dt,mode", LZ_CASES, ids=["n%d-q%d-b%d-%s-%s" % c for c in LZ_CASES])
def test_lanczos_pieces_on_framed_poisoned_exact_buffers(n, q, nb, dt, mode):
    tdt, npdt, _ = DT[dt]
    reorth, slots = LZ_MODES[mode]
    case = _lz_case(n, q, nb, dt, reorth)
    rows, cols, _, _, _, pat = _tri_case(n)
    sol, prod = pat.solver, pat.product
    nq, stride = n * q, n * q + PAD
    W = D.work_bytes(sol, "lanczos", n, q, KMAX)
    blen = (slots - 1) * stride + nq                       # the last slot ends the array: no spare gap behind it
    buf = Buffers(npdt, nb, {"values": len(rows), "v0": nq, "w": nq, "basis": blen},
                  {"state": nb * q * 12, "coef": nb * q * 2 * KMAX}, {"work": W * nb})
    for m, c in enumerate(case):
        buf.fill("values", m, c["values"])
        buf.fill("v0", m, c["v0"])
    watched = ("basis", "state", "coef")
    buf.seal(watched)
    seen = []

    def hook(piece, step, info):
        torch.cuda.synchronize()
        what = "%s at step %d" % (piece, step)
        writes = D.PRODUCT_WRITES["lanczos"] if piece == "mv" else D.write_set(piece, fold=info.get("fold", False))
        writes = tuple("basis" if w == "slot" else w for w in writes)
        buf.assert_frames(writes, what)
        cur = buf.snapshot(watched)
        was = buf.prev["state"].view(np.int64).reshape(nb, q, 12)
        now = cur["state"].view(np.int64).reshape(nb, q, 12)
        cwas = buf.prev["coef"].view(np.int64).reshape(nb, q, 2, KMAX)
        cnow = cur["coef"].view(np.int64).reshape(nb, q, 2, KMAX)
        for m in range(nb):
            if piece == "lanczos_init":
                assert not (now[m] == POISON64).any(), (what, m, "a word of a record was not written")
                stopped = now[m, :, 1] != LR.RUNNING           # a zero start vector writes no slot
            else:
                stopped = was[m, :, 1] != LR.RUNNING
                assert (was[m][stopped] == now[m][stopped]).all(), (what, m, "the record of a stopped problem changed")
            if "basis" in writes:
                s0 = info["slot"] * stride
                a, b = _words(buf.prev["basis"][m]), _words(cur["basis"][m])
                outside = np.ones(blen, dtype=bool)
                outside[s0:s0 + nq] = False
                assert (a[outside] == b[outside]).all(), (what, m, "another slot, or a gap between slots, was written")
                _frozen_columns(a[s0:s0 + nq], b[s0:s0 + nq], stopped, q, (what, "slot %d" % info["slot"], m))
            if "coef" in writes:
                for c in range(q):
                    free = np.zeros((2, KMAX), dtype=bool)
                    if not stopped[c]:
                        free[:, was[m, c, 0]] = True       # entry j of alpha and of beta, j = the steps done
                    assert (cwas[m, c][~free] == cnow[m, c][~free]).all(), (what, m, c, "a coefficient of another step")
        buf.seal(watched)
        seen.append(piece)

    basis = buf.op("basis")
    ops = {"values": buf.op("values"), "v0": [t.view(n, q) for t in buf.op("v0")], "w": [t.view(n, q) for t in buf.op("w")],
           "basis": basis}
    run = D.LanczosPieces(sol, prod, dt, n, q, KMAX, nb, nb > 1, ops, stride, slots, buf.addr("coef"), buf.addr("work"),
                          buf.addr("state"), full=reorth == "full", hook=hook,
                          slot_view=lambda m, s: basis[m][s * stride:s * stride + nq].view(n, q))
    run.run()
    want_pieces = {"mv", "lanczos_init", "lanczos_alpha", "lanczos_update", "lanczos_normalize"}
    want_pieces |= {"lanczos_project", "lanczos_subtract"} if reorth == "full" else set()
    assert set(seen) == want_pieces and seen.count("lanczos_update") == KMAX

    state = buf.host("state").view(np.int64).reshape(nb, q, 12)
    coef = buf.host("coef").reshape(nb, q, 2, KMAX)
    done = []
    for m, c in enumerate(case):
        st, V = c["st"], c["V"]
        got = buf.host("basis", m)
        gaps = np.ones(blen, dtype=bool)
        for s in range(slots):
            gaps[s * stride:s * stride + nq] = False
        assert is_sentinel(got[gaps]).all(), (m, "a gap between slots was written")
        for j in range(q):
            np.testing.assert_array_equal(state[m, j], LR.record_words(st, j), err_msg="member %d column %d" % (m, j))
            k = int(st["steps"][j])
            assert _same(coef[m, j, :, :k], c["coef"][j, :, :k]), (m, j, "alpha / beta are not the restatement's")
            assert is_sentinel(coef[m, j, :, k:]).all(), (m, j, "a coefficient beyond the steps done was written")
            # column j wrote v_0 .. v_{k-1} (v_k is not formed once the problem has stopped); slot s holds the last
            # of them that maps to it
            holds = {}
            for i in range(min(k, KMAX)):
                holds[i if slots == KMAX else i % 2] = i
            for s in range(slots):
                col = got[s * stride:s * stride + nq].reshape(n, q)[:, j]
                if s in holds:
                    assert _same(col, V[holds[s]][:, j]), (m, j, "slot %d is not v_%d" % (s, holds[s]))
                else:
                    assert is_sentinel(col).all(), (m, j, "slot %d was written" % s)
        done += st["steps"].tolist()
    if n > 1 and (q == 3 or nb == 2):
        assert 0 < min(d for d in done if d > 0) < KMAX == max(done), ("no problem stopped early beside one that ran on", done)
    if q == 3:
        assert all(c["st"]["stop"][2] == LR.ZERO_START for c in case)


# ---- n = 0: the pieces that need no map --------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", [1, 3])
def test_empty_problems_write_their_record_and_nothing_else(q, dt):
    sol = _tri_case(1)[5].solver
    lib = sol._lib
    Wc, Wl = D.work_bytes(sol, "cg", 0, q), D.work_bytes(sol, "lanczos", 0, q, 4)
    words = Frame([q * 12, q * 12, q * 2 * 4], np.float64, guard=GUARD)
    work = Frame([Wc // 8, Wl // 8], np.float64, guard=GUARD, align_bytes=16)
    cg_state, lz_state, coef = (words.view(k).data_ptr() for k in range(3))
    N0, Q = I64(0), I64(q)
    tail = (P(work.view(0).data_ptr()), P(cg_state))
    f = lambda name: getattr(lib, "bsp_" + name + "_" + dt)
    err = lambda: lib.bsp_last_error().decode()
    assert f("cg_init")(sol._h, N0, Q, None, None, None, F64(1e-3), I64(7), I32(1), *tail) == 0, err()
    torch.cuda.synchronize()
    words.assert_intact()
    work.assert_intact()
    want = np.zeros(12, dtype=np.int64)
    want[1], want[9] = R.ZERO_RHS, 7
    want[8:9] = np.array([1e-3 * 1e-3]).view(np.int64)
    rec = words.host(0).view(np.int64).reshape(q, 12)
    assert (rec == want).all(), rec
    assert is_sentinel(words.host(1)).all() and is_sentinel(words.host(2)).all() and is_sentinel(work.host(1)).all()
    words.seal()
    assert f("cg_alpha")(sol._h, N0, Q, None, None, *tail) == 0, err()
    assert f("cg_update")(sol._h, N0, Q, None, None, None, None, I32(1), *tail) == 0, err()
    assert f("cg_direction")(sol._h, N0, Q, None, None, I32(1), *tail) == 0, err()
    torch.cuda.synchronize()
    words.assert_intact(read_only=[0, 1, 2], what="alpha, update, direction at n = 0")
    work.assert_intact()
    assert f("lanczos_init")(sol._h, N0, Q, I64(4), None, None, I64(0), I64(1), I64(0), F64(0.25),
                             P(work.view(1).data_ptr()), P(lz_state)) == 0, err()
    torch.cuda.synchronize()
    words.assert_intact(read_only=[0, 2], what="lanczos_init at n = 0")
    work.assert_intact()
    want = np.zeros(12, dtype=np.int64)
    want[1], want[7] = LR.ZERO_START, 4
    want[6:7] = np.array([0.25 * 0.25]).view(np.int64)
    rec = words.host(1).view(np.int64).reshape(q, 12)
    assert (rec == want).all(), rec
    assert is_sentinel(words.host(2)).all(), "the coefficients of a problem that took no step"


# ---- the error-bound calls not yet framed ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_inv_norm1_batched_in_frames(dt):
    tdt, npdt, _ = DT[dt]
    pat, A, vals = _pattern_of("grid8", "scalar")
    sol, lib = pat.solver, pat.solver._lib
    scales = [1.0, 1.5, 0.25]
    nb = len(scales)
    L = _factor(pat, np.stack([vals * s for s in scales]), tdt)
    need = ctypes.c_int64(0)
    assert getattr(lib, "bsp_inv_norm1_work_bytes_" + dt)(sol._h, ctypes.byref(need)) == 0 and need.value % 16 == 0
    work = Frame([need.value * nb // 8], np.float64, guard=GUARD, align_bytes=16)
    words = Frame([nb * 12, nb], np.float64, guard=GUARD)    # state and out inside a larger tensor, at odd offsets
    ptrs = (ctypes.c_void_p * nb)(*[L[m].data_ptr() for m in range(nb)])
    keep = L.clone()
    rc = getattr(lib, "bsp_inv_norm1_batched_" + dt)(sol._h, ptrs, None, P(work.view(0).data_ptr()),
                                                      P(words.view(0).data_ptr()), P(words.view(1).data_ptr()), I32(nb))
    assert rc == 0, lib.bsp_last_error().decode()
    torch.cuda.synchronize()
    work.assert_intact(what="the work of %d members, exactly %d bytes each" % (nb, need.value))
    words.assert_intact()
    assert torch.equal(L, keep), "a factor was written"
    out = words.host(1)
    state = words.host(0).view(np.int64).reshape(nb, 12)
    assert not is_sentinel(words.host(0)).any() and (state[:, 11] == 0).all()
    n = A.shape[0]
    for m, s in enumerate(scales):
        true = E.true_inv_norm1(A) / s
        assert true / 3 <= out[m] <= true * (1 + n * E.kappa1(A) * np.finfo(npdt).eps), (m, out[m], true)
        assert state[m, 0] == out[m:m + 1].view(np.int64)[0], "word 0 of the record is the estimate"
        one = float(sol.invNorm1(L[m]))
        assert abs(out[m] - one) <= n * E.kappa1(A) * np.finfo(npdt).eps * one, (m, out[m], one)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_max_ratio_and_col_max_write_a_framed_out(dt):
    tdt, npdt, _ = DT[dt]
    sol = _tri_case(1)[5].solver
    lib = sol._lib
    rng = np.random.default_rng(46)
    for nb, n, q in ((1, 1, 1), (2, 1025, 3), (3, 255, 1), (2, 2049, 3)):
        r = rng.standard_normal((nb, n, q)).astype(npdt)
        d = rng.uniform(0.1, 2, (nb, n, q)).astype(npdt)
        r[0, rng.integers(n)] = 0
        fr = framed(npdt, [r[m] for m in range(nb)] + [d[m] for m in range(nb)], guard=GUARD)
        out = Frame([nb * q, nb * q], np.float64, guard=GUARD)
        rp = (ctypes.c_void_p * nb)(*[fr.view(m).data_ptr() for m in range(nb)])
        dp = (ctypes.c_void_p * nb)(*[fr.view(nb + m).data_ptr() for m in range(nb)])
        assert getattr(lib, "bsp_max_ratio_batched_" + dt)(sol._h, rp, dp, I64(n), I64(q), P(out.view(0).data_ptr()),
                                                            I32(nb)) == 0, lib.bsp_last_error().decode()
        assert getattr(lib, "bsp_col_max_batched_" + dt)(sol._h, rp, I64(n), I64(q), P(out.view(1).data_ptr()),
                                                          I32(nb)) == 0, lib.bsp_last_error().decode()
        torch.cuda.synchronize()
        fr.assert_intact(read_only=range(2 * nb), what=(nb, n, q))
        out.assert_intact(what=(nb, n, q))
        ratio, cmax = out.host(0).reshape(nb, q), out.host(1).reshape(nb, q)
        for m in range(nb):
            assert _same(ratio[m], np.asarray(E.max_ratio(r[m], d[m]))), (dt, nb, n, q, m)
            assert _same(cmax[m], np.asarray(E.col_max(r[m]))), (dt, nb, n, q, m)
