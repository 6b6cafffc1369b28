"""baspacho_amd -- MI355X-native supernodal sparse Cholesky (host-side Python mirror).

Thin mirror of the reference's public C++ surface (baspacho/baspacho/Solver.h) over the C ABI
of the HIP library (include/baspacho_amd.h): `create_solver`, `Solver.factor/solve`, block
accessors, skeleton arrays.  PyTorch is only plumbing here (device memory, streams,
torch.distributed); numeric work happens in the hand-written HIP kernels.
"""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib

__all__ = ["Settings", "Solver", "FactorizationError", "Assembly", "NormalEquations", "JacobianProduct", "JacobianSchur", "SymProduct", "create_solver", "SparseStructure", "BackendHip", "BackendCuda",
           "BackendRef", "BackendFast", "AddFillComplete", "AddFillForAutoElims",
           "AddFillForGivenElims", "AddFillNone"]

# Solver.h:189-209
BackendRef, BackendFast, BackendCuda, BackendHip = 0, 1, 2, 3
AddFillComplete, AddFillForAutoElims, AddFillForGivenElims, AddFillNone = 0, 1, 2, 3

_I64P = ctypes.POINTER(ctypes.c_int64)

_SKEL_IDS = {
    "spanStart": 0, "spanToLump": 1, "lumpStart": 2, "lumpToSpan": 3, "spanOffsetInLump": 4,
    "chainColPtr": 5, "chainRowSpan": 6, "chainData": 7, "chainRowsTillEnd": 8,
    "boardColPtr": 9, "boardRowLump": 10, "boardChainColOrd": 11, "boardRowPtr": 12,
    "boardColLump": 13, "boardColOrd": 14,
}

PROF_KINDS = ["elim_factor", "elim_update", "potrf", "trsm", "update", "chain_update"]


class _CSettings(ctypes.Structure):
    _fields_ = [("find_sparse_elimination_ranges", ctypes.c_int32),
                ("num_threads", ctypes.c_int32), ("backend", ctypes.c_int32),
                ("add_fill_policy", ctypes.c_int32),
                ("computation_model", ctypes.POINTER(ctypes.c_double))]


_HIP_OPTION_INTS = ["lookahead", "due_stream", "split_k", "gather_max_pairs",
                    "sub_batch_min", "sub_batches", "tail_blocks", "lazy_plan", "block_solve", "solve_inv",
                    "solve_sweep", "sweep_min_width", "solve_wide", "chain_contraction", "dense_merge", "expected_batch"]
_HIP_OPTION_REALS = ["lookahead_min_gf", "bulk_ahead", "level_cost_us"]


class _CHipOptions(ctypes.Structure):
    """bsp_hip_options (include/baspacho_amd.h): negative / NaN = the library's default"""
    # (gather_overlap: ignored by the library, kept for ABI stability; a slot, not an option)
    _fields_ = [(n, ctypes.c_int32) for n in _HIP_OPTION_INTS[:4] + ["gather_overlap"] + _HIP_OPTION_INTS[4:]] + \
               [(n, ctypes.c_double) for n in _HIP_OPTION_REALS]


class _CPlanStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in
                ["flops", "upd_elems", "upd_flops", "elim_pair_elems", "elim_pair_flops",
                 "elim_col_elems", "upd_flops_direct", "elim_pair_operand_elems",
                 "elim_target_elems", "trsm_flops", "potrf_flops", "trsm_flops_merged",
                 "potrf_flops_fused"]] + \
               [(n, ctypes.c_int64) for n in
                ["num_launches", "num_levels", "num_panels", "num_segs", "num_upd_tasks",
                 "num_trsm_tasks", "chain_tab_entries", "max_panels_in_level",
                 "num_atomic_upd_tasks", "num_gather_groups", "num_fork_levels"]] + \
               [("deferred_flops", ctypes.c_double), ("tail_upd_flops", ctypes.c_double),
                ("num_tail_panels", ctypes.c_int64)]


class _CRunCounters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in
                ["sweep_launches", "sweep_timeouts", "split_lists_used", "sub_batches_enqueued",
                 "lookahead_forks", "sweeps_retired", "sweep_error_pending",
                 "gather_chunks_overlapped", "tail_launches", "sweep_mfma_launches",
                 "solve_wide_launches", "inv_reused", "potrf_folded_levels", "selinv_launches",
                 "selinv_chunks"]]


@dataclass
class Settings:
    """Solver.h:212-218"""
    findSparseEliminationRanges: bool = True
    numThreads: int = 16
    backend: int = BackendHip
    addFillPolicy: int = AddFillComplete
    computationModel: Optional[Sequence[float]] = None  # 20 coefficients, see C header
    # extension: schedule switches of the MI355X backend, {field of bsp_hip_options: value}; fields left
    # out keep the library's default (the BSP_* environment variables override both, for A/B scripts)
    hipOptions: Optional[dict] = None


@dataclass
class SparseStructure:
    """block CSR pattern (lower triangle incl. diagonal); SparseStructure.h:19-29"""
    ptrs: np.ndarray
    inds: np.ndarray

    def __post_init__(self):
        self.ptrs = np.ascontiguousarray(self.ptrs, dtype=np.int64)
        self.inds = np.ascontiguousarray(self.inds, dtype=np.int64)

    def order(self):
        return len(self.ptrs) - 1

    # SparseStructure.h:34-55 (executed by the C++ host library)
    def transpose(self):
        return _ss_op(self, SS_TRANSPOSE)

    def clear(self, clearLower=True):
        return _ss_op(self, SS_CLEAR, flag=int(clearLower))

    def symmetricPermutation(self, mapPerm, lowerHalf=True):
        return _ss_op(self, SS_SYM_PERMUTATION, mapPerm, int(lowerHalf))

    def addIndependentEliminationFill(self, start, end):
        return _ss_op(self, SS_INDEP_ELIM_FILL, [start, end])

    def addFullEliminationFill(self):
        return _ss_op(self, SS_FULL_ELIM_FILL)

    def fillReducingPermutation(self):
        return _ss_op(self, SS_FILL_REDUCING_PERM)

    def extractRightBottom(self, start):
        return _ss_op(self, SS_EXTRACT_RIGHT_BOTTOM, [start])


SS_TRANSPOSE, SS_CLEAR, SS_SYM_PERMUTATION, SS_INDEP_ELIM_FILL, SS_FULL_ELIM_FILL, \
    SS_FILL_REDUCING_PERM, SS_EXTRACT_RIGHT_BOTTOM = range(7)


def _ss_op(ss, op, arg=(), flag=0):
    lib = _lib.load()
    n = ss.order()
    a = _i64(arg)
    cap = max(16, 4 * len(ss.inds) + n)
    while True:
        out_ptrs = np.zeros(n + 2, dtype=np.int64)
        out_inds = np.zeros(cap, dtype=np.int64)
        on, onnz = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = lib.bsp_sparse_structure_op(
            op, ctypes.c_int64(n), ss.ptrs.ctypes.data_as(_I64P), ss.inds.ctypes.data_as(_I64P),
            a.ctypes.data_as(_I64P), ctypes.c_int64(len(a)), ctypes.c_int32(flag),
            out_ptrs.ctypes.data_as(_I64P), out_inds.ctypes.data_as(_I64P), ctypes.c_int64(cap),
            ctypes.byref(on), ctypes.byref(onnz))
        if rc != 0 and onnz.value > cap:
            cap = onnz.value
            continue
        _check(rc)
        if op == SS_FILL_REDUCING_PERM:
            return out_inds[:onnz.value].copy()
        return SparseStructure(out_ptrs[:on.value + 1].copy(), out_inds[:onnz.value].copy())


def _check(rc):
    if rc != 0:
        raise RuntimeError(_lib.load().bsp_last_error().decode("utf-8", "replace"))


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptr_of(t):
    """device pointer of a torch tensor (or a raw int address)"""
    if isinstance(t, int):
        return t
    if not t.is_cuda:
        raise ValueError("numeric data must live in device memory (Solver.h:184-188)")
    if not t.is_contiguous():
        raise ValueError("numeric data must be contiguous")
    return t.data_ptr()


def _suffix(t):
    import torch
    if t.dtype == torch.float64:
        return "f64"
    if t.dtype == torch.float32:
        return "f32"
    raise TypeError("only float64 / float32 data is supported, got %s" % t.dtype)


def _ptr_array(tensors):
    """host array of the device pointers of `tensors`, one per batch member (None: a NULL array)"""
    if tensors is None:
        return None
    return (ctypes.c_void_p * len(tensors))(*[_ptr_of(t) for t in tensors])


def _ptr_arg(members, batched):
    """a pointer argument of an entry that has a batched form: the pointer array of the members for a
    batch, the pointer of the one member else (None: NULL either way)"""
    if members is None:
        return None
    return _ptr_array(members) if batched else ctypes.c_void_p(_ptr_of(members[0]))


def _count(members, batched):
    """the batch-size argument of a batched entry (none for a single call)"""
    return (ctypes.c_int32(len(members)),) if batched else ()


def _call(lib, name, batched, sfx, *args):
    """call `name` + ["batched_"] + sfx, the single or the batched entry of one operation; raises the
    library's error"""
    _check(getattr(lib, name + ("batched_" if batched else "") + sfx)(*args))


class FactorizationError(RuntimeError):
    """A factor broke down and the regularised retries ran out (Solver.factorRegularized).  `status` is
    the decoded record of the last try of the (first) failing matrix, `info` what factorRegularized
    would have returned"""

    def __init__(self, message, status, info=None):
        super().__init__(message)
        self.status = status
        self.info = info


class Solver:
    """Mirror of BaSpaCho::Solver (Solver.h:34-180).  Do not construct directly: use
    `create_solver`, `Solver.from_skeleton` or `Solver.from_plan`."""

    def __init__(self, handle):
        self._lib = _lib.load()
        self._h = handle
        self._skel = None
        self._stream = None  # what setStream() was last given (the autograd functions restore it)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.bsp_destroy_solver(h)

    # ---- construction -------------------------------------------------------------------
    @staticmethod
    def from_skeleton(span_start, lump_to_span, col_ptr, row_ind, sparse_elim_ranges=()):
        """Solver(CoalescedBlockMatrixSkel&&, sparseElimRanges, {}, ops)  (Solver.h:37-38)"""
        lib = _lib.load()
        ss, l2s, cp, ri = _i64(span_start), _i64(lump_to_span), _i64(col_ptr), _i64(row_ind)
        er = _i64(sparse_elim_ranges)
        h = ctypes.c_void_p()
        _check(lib.bsp_create_solver_from_skeleton(
            ctypes.c_int64(len(ss) - 1), ss.ctypes.data_as(_I64P), ctypes.c_int64(len(l2s) - 1),
            l2s.ctypes.data_as(_I64P), cp.ctypes.data_as(_I64P), ri.ctypes.data_as(_I64P),
            ctypes.c_int64(len(er)), er.ctypes.data_as(_I64P), ctypes.byref(h)))
        return Solver(h)

    @staticmethod
    def from_plan(buf):
        """rebuild a solver from `serialize_plan()` output (e.g. after an RCCL broadcast)"""
        lib = _lib.load()
        b = _i64(buf)
        h = ctypes.c_void_p()
        _check(lib.bsp_create_solver_from_plan(b.ctypes.data_as(_I64P), ctypes.c_int64(len(b)),
                                               ctypes.byref(h)))
        return Solver(h)

    def serialize_plan(self):
        need = ctypes.c_int64(0)
        _check(self._lib.bsp_plan_serialize(self._h, None, ctypes.c_int64(0), ctypes.byref(need)))
        buf = np.empty(need.value, dtype=np.int64)
        _check(self._lib.bsp_plan_serialize(self._h, buf.ctypes.data_as(_I64P), need,
                                            ctypes.byref(need)))
        return buf

    # ---- sizes / structure --------------------------------------------------------------
    def order(self):
        return int(self._lib.bsp_order(self._h))

    def dataSize(self):
        return int(self._lib.bsp_data_size(self._h))

    def canFactorUpToSpan(self):
        return int(self._lib.bsp_can_factor_up_to_span(self._h))

    def numSpans(self):
        return int(self._lib.bsp_num_spans(self._h))

    def numLumps(self):
        return int(self._lib.bsp_num_lumps(self._h))

    def spanVectorOffset(self, span):
        return int(self._lib.bsp_span_vector_offset(self._h, ctypes.c_int64(span)))

    def spanMatrixOffset(self, span):
        out = ctypes.c_int64(0)
        _check(self._lib.bsp_span_matrix_offset(self._h, ctypes.c_int64(span), ctypes.byref(out)))
        return out.value

    def _array(self, which):
        p, n = _I64P(), ctypes.c_int64(0)
        _check(self._lib.bsp_skeleton_array(self._h, which, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int64)
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy()

    def skel(self):
        """dict of the CoalescedBlockMatrixSkel arrays (CoalescedBlockMatrix.h:88-110)"""
        if self._skel is None:
            self._skel = {k: self._array(v) for k, v in _SKEL_IDS.items()}
        return self._skel

    def paramToSpan(self):
        return self._array(15)

    def sparseEliminationRanges(self):
        return self._array(16)

    # ---- accessors ----------------------------------------------------------------------
    def blockOffset(self, row_param, col_param):
        """(offset, stride, flipped)  -- PermutedCoalescedAccessor::blockOffset"""
        off, st, fl = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        _check(self._lib.bsp_block_offset(self._h, ctypes.c_int64(row_param),
                                          ctypes.c_int64(col_param), ctypes.byref(off),
                                          ctypes.byref(st), ctypes.byref(fl)))
        return off.value, st.value, bool(fl.value)

    def diagBlockOffset(self, param):
        off, st = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self._lib.bsp_diag_block_offset(self._h, ctypes.c_int64(param), ctypes.byref(off),
                                               ctypes.byref(st)))
        return off.value, st.value

    def diagBlockOffsetOfSpan(self, span):
        """(offset, stride) of the diagonal block of a SPAN (internal order), from the skeleton:
        CoalescedAccessor::diagBlockOffset (Accessor.h:75-85)"""
        sk = self.skel()
        lump = int(sk["spanToLump"][span])
        idx = span - int(sk["lumpToSpan"][lump])
        off = int(sk["chainData"][int(sk["chainColPtr"][lump]) + idx]) + int(sk["spanOffsetInLump"][span])
        return off, int(sk["lumpStart"][lump + 1] - sk["lumpStart"][lump])

    def deviceAccessor(self):
        """8 device addresses (spanStart, spanToLump, lumpStart, spanOffsetInLump, chainColPtr,
        chainRowSpan, chainData, permutation) usable from a caller's HIP kernel"""
        arr = (_I64P * 8)()
        _check(self._lib.bsp_device_accessor(self._h, arr))
        return [ctypes.cast(a, ctypes.c_void_p).value for a in arr]

    # ---- numeric ------------------------------------------------------------------------
    def setStream(self, stream):
        """stream: torch.cuda.Stream, raw hipStream_t address, or None (default stream)"""
        addr = 0 if stream is None else getattr(stream, "cuda_stream", stream)
        self._lib.bsp_set_stream(self._h, ctypes.c_void_p(addr))
        self._stream = stream

    def _check_data(self, t):
        if t.numel() != self.dataSize():
            raise ValueError("data has %d elements, factor needs %d" % (t.numel(), self.dataSize()))

    def factor(self, data):
        """Solver::factor<T> / factor<std::vector<T*>> (list/tuple of tensors = batch)"""
        if isinstance(data, (list, tuple)):
            sfx = _suffix(data[0])
            for t in data:
                self._check_data(t)
            ptrs = _ptr_array(data)
            _check(getattr(self._lib, "bsp_factor_batched_" + sfx)(self._h, ptrs,
                                                                   ctypes.c_int32(len(data))))
        else:
            self._check_data(data)
            _check(getattr(self._lib, "bsp_factor_" + _suffix(data))(
                self._h, ctypes.c_void_p(_ptr_of(data))))

    def factorPerOp(self, data):
        """TESTING: factor() through the per-op NumericCtx boundary in the reference's call order"""
        self._check_data(data)
        _check(getattr(self._lib, "bsp_factor_per_op_" + _suffix(data))(
            self._h, ctypes.c_void_p(_ptr_of(data))))

    def forcePerOp(self, on=True):
        """TESTING: route factor / solve* / addMvFrom through the reference's per-op NumericCtx /
        SolveCtx boundary (bsp_force_per_op); usable as a context manager"""
        _check(self._lib.bsp_force_per_op(self._h, ctypes.c_int32(1 if on else 0)))
        solver = self

        class _Scope:
            def __enter__(self_inner):
                return solver

            def __exit__(self_inner, *exc):
                _check(solver._lib.bsp_force_per_op(solver._h, ctypes.c_int32(0)))
                return False
        return _Scope()

    def _testSetFault(self, kind):
        """TESTING, fault injection (bsp_test_set_fault): 1 = factor() skips the sparse-elimination
        update, 0 = off"""
        _check(self._lib.bsp_test_set_fault(self._h, ctypes.c_int32(kind)))

    def _testSetSelInvBatchChunk(self, max_matrices):
        """TESTING: at most `max_matrices` matrices per chunk of a batched selectedInverse
        (bsp_test_set_selinv_batch_chunk); 0 = the product's rule"""
        _check(self._lib.bsp_test_set_selinv_batch_chunk(self._h, ctypes.c_int32(max_matrices)))

    def _testPtrRingSlotBytes(self):
        """TESTING, read-only: bytes of one slot of the pointer ring of batched calls
        (bsp_test_ptr_ring_slot_bytes); 0 before the first batched call"""
        out = ctypes.c_int64(0)
        _check(self._lib.bsp_test_ptr_ring_slot_bytes(self._h, ctypes.byref(out)))
        return int(out.value)

    _SELINV_SMALL_FIELDS = ("lump", "level", "n", "r", "k")
    _SELINV_NODE_FIELDS = ("lump", "level", "c0", "w", "r", "nRest", "kChunk", "nk", "nTiles", "tileBase")

    def _testSelInvPlan(self, upToSpan=None):
        """TESTING: the selected-inversion plan of this solver (bsp_test_selinv_plan, built on the host
        by the function selectedInverse() uses).  {"numLevels", "linvElems", "uElems", "pElems",
        "wElems": int, "small": {field: int64 array}, "node": {field: int64 array}}, records in launch
        order; small fields lump, level, n, r, k; node fields lump, level, c0, w, r, nRest, kChunk, nk,
        nTiles, tileBase.  upToSpan: the plan of the lumps before that span alone, which
        factorAdjointUpTo runs (bsp_test_selinv_plan_up_to)"""
        if upToSpan is None:
            def call(buf, cap, need):
                return self._lib.bsp_test_selinv_plan(self._h, buf, cap, need)
        else:
            def call(buf, cap, need):
                return self._lib.bsp_test_selinv_plan_up_to(self._h, ctypes.c_int64(upToSpan), buf, cap, need)
        need = ctypes.c_int64(0)
        _check(call(None, ctypes.c_int64(0), ctypes.byref(need)))
        buf = np.empty(need.value, dtype=np.int64)
        _check(call(buf.ctypes.data_as(_I64P), need, ctypes.byref(need)))
        nlev, ns, nn = (int(x) for x in buf[:3])
        out = {"numLevels": nlev, "linvElems": int(buf[3]), "uElems": int(buf[4]), "pElems": int(buf[5]),
               "wElems": int(buf[6])}
        fs, fn = self._SELINV_SMALL_FIELDS, self._SELINV_NODE_FIELDS
        sm = buf[7:7 + ns * len(fs)].reshape(ns, len(fs))
        nd = buf[7 + ns * len(fs):].reshape(nn, len(fn))
        out["small"] = {f: sm[:, i].copy() for i, f in enumerate(fs)}
        out["node"] = {f: nd[:, i].copy() for i, f in enumerate(fn)}
        return out

    def _testReachPlan(self, params):
        """TESTING: the reach plan of `params` (caller's ids) with one Gram item per pair (i, j), i >= j,
        of their positions (bsp_test_reach_plan, built on the host by the function inverseBlocks() uses).
        {"cutLump", "cutSpan", "numCols": int, "queries": [{"span", "lump", "col0", "width", "reach":
        int64 array (truncated at the cut)}], "groups": [{"query", "col0", "k", "row0", "len",
        "firstLump"}], "items": [{"i", "j", "colP", "nP", "colQ", "nQ", "outOff", "rows", "ranges":
        [(begin, end)] internal scalars}], "units": [(column, row)]}"""
        prm = _i64(list(params))
        buf = self._testRecords(lambda b, cap, need: self._lib.bsp_test_reach_plan(
            self._h, ctypes.c_int64(len(prm)), prm.ctypes.data_as(_I64P), b, cap, need))
        cut, cut_span, ncols, nq, ng, ni, nu = (int(x) for x in buf[:7])
        pos = 7
        out = {"cutLump": cut, "cutSpan": cut_span, "numCols": ncols, "queries": [], "groups": [], "items": []}
        for _ in range(nq):
            span, lump, col0, width, ln = (int(x) for x in buf[pos:pos + 5])
            out["queries"].append({"span": span, "lump": lump, "col0": col0, "width": width,
                                   "reach": buf[pos + 5:pos + 5 + ln].copy()})
            pos += 5 + ln
        for _ in range(ng):
            out["groups"].append(dict(zip(("query", "col0", "k", "row0", "len", "firstLump"),
                                          (int(x) for x in buf[pos:pos + 6]))))
            pos += 6
        for _ in range(ni):
            it = dict(zip(("i", "j", "colP", "nP", "colQ", "nQ", "outOff", "rows"), (int(x) for x in buf[pos:pos + 8])))
            nr = int(buf[pos + 8])
            it["ranges"] = [(int(a), int(b)) for a, b in buf[pos + 9:pos + 9 + 2 * nr].reshape(nr, 2)]
            out["items"].append(it)
            pos += 9 + 2 * nr
        out["units"] = [(int(a), int(b)) for a, b in buf[pos:pos + 2 * nu].reshape(nu, 2)]
        assert pos + 2 * nu == len(buf)
        return out

    def _testFactorProductPlan(self):
        """TESTING: the plan of mulL / mulLt (bsp_test_factor_product_plan, built on the host by the
        function the products use).  {"partElems": int; int64 arrays "spanChainPtr", "spanChain",
        "spanChainLump", "spanLong", "longRows", "smallColLump", "smallCol", "hugeSpans", "hugeWidePtr",
        "hugeWide"; "tasks": {"dataOff", "lump", "w", "c0", "nc", "rBeg", "rEnd", "chain", "part"}, "folds":
        {"col0", "nc", "part0", "numChunks"}: one int64 array per field}"""
        buf = self._testRecords(lambda b, cap, need: self._lib.bsp_test_factor_product_plan(self._h, b, cap, need))
        ns, nc, nl, nt, nf, nsm, part, nh, nhw = (int(x) for x in buf[:9])
        out = self._testSplitRecords(buf, 9, [
            ("spanChainPtr", ns + 1, None), ("spanChain", nc, None), ("spanChainLump", nc, None),
            ("spanLong", ns, None), ("longRows", nl, None),
            ("tasks", nt, ("dataOff", "lump", "w", "c0", "nc", "rBeg", "rEnd", "chain", "part")),
            ("folds", nf, ("col0", "nc", "part0", "numChunks")),
            ("smallColLump", nsm, None), ("smallCol", nsm, None),
            ("hugeSpans", nh, None), ("hugeWidePtr", nh + 1, None), ("hugeWide", nhw, None)])
        out["partElems"] = part
        return out

    def _testRecords(self, call):
        need = ctypes.c_int64(0)
        _check(call(None, ctypes.c_int64(0), ctypes.byref(need)))
        buf = np.empty(need.value, dtype=np.int64)
        _check(call(buf.ctypes.data_as(_I64P), need, ctypes.byref(need)))
        return buf

    @staticmethod
    def _testSplitRecords(buf, pos, tables):
        """consecutive tables of `buf` from `pos` on: (name, rows, field names or None for a plain array)"""
        out = {}
        for name, rows, fields in tables:
            if fields is None:
                out[name] = buf[pos:pos + rows].copy()
                pos += rows
            else:
                t = buf[pos:pos + rows * len(fields)].reshape(rows, len(fields))
                out[name] = {f: t[:, i].copy() for i, f in enumerate(fields)}
                pos += rows * len(fields)
        assert pos == len(buf)
        return out

    _PANEL_FIELDS = ("diagOff", "lda", "nb", "rowsBelow", "nRest", "lumpRowBase", "lump", "vecOff")
    _WIDE_FIELDS = ("srcOff", "tgtBase", "chainTabPtr", "lda", "K", "rowsBelow", "nRest", "lumpRowBase", "kind",
                    "segEnd", "tgtStride", "firstChainOrd", "rowMin", "rowTile", "colTile", "atomic")

    def _testLaunchTables(self):
        """TESTING: the launch tables of the factor plan over every lump (bsp_test_launch_tables, built on
        the host by the function the launch code uses).  {"numMainLevels", "numLevelPanels",
        "numTrsmTasks", "numUpdTasks": int (of the plan), table name: {field: int64 array} or int64 array};
        "levels" lists the bigLevels of every elimination range, then the plan's own levels (range -1)"""
        buf = self._testRecords(lambda b, cap, need: self._lib.bsp_test_launch_tables(self._h, b, cap, need))
        n = [int(v) for v in buf[:16]]
        out = self._testSplitRecords(buf, 16, (
            ("levels", n[0], ("range", "tail", "directPanel", "panelBegin", "panelEnd", "trsmBegin", "trsmEnd",
                              "updBegin", "updEnd")),
            ("levelPanelDescs", n[5], self._PANEL_FIELDS),
            ("trsmTasksFat", n[6], ("diagOff", "lda", "nb", "rowsBelow", "rowTile")),
            ("updTasksFat", n[7], ("srcOff", "tgtBase", "lda", "K", "rowsBelow", "segEnd", "rowTile", "colTile",
                                   "tgtStride", "rowMin", "atomic", "fast")),
            ("updTasksWide", n[8], self._WIDE_FIELDS),
            ("slowPrefix", n[9], None),
            ("updTasksSplit", n[10], self._WIDE_FIELDS),
            ("splitRange", n[11], ("updBegin", "begin", "end")),
            ("foldRank", n[12], None), ("foldTiles", n[13], None), ("foldPanelEnd", n[14], None),
            ("foldDescs", n[15], self._PANEL_FIELDS)))
        out.update(numMainLevels=n[1], numLevelPanels=n[2], numTrsmTasks=n[3], numUpdTasks=n[4])
        return out

    def _testSolveSchedule(self, withSweeps, blockSolve, inverses, sweepMinWidth=768):
        """TESTING: the solve schedule of the same plan's own levels under the given switches
        (bsp_test_solve_schedule).  {"numSweeps", "sweepInstStride", "maxSweepWgs", "maxSweepWgsM",
        "maxSweepW", "maxSweepBelow": int, "levels", "items", "invPanels": {field: int64 array}}"""
        buf = self._testRecords(lambda b, cap, need: self._lib.bsp_test_solve_schedule(
            self._h, ctypes.c_int32(int(withSweeps)), ctypes.c_int32(int(blockSolve)), ctypes.c_int32(int(inverses)),
            ctypes.c_int32(sweepMinWidth), b, cap, need))
        n = [int(v) for v in buf[:9]]
        panel = ("lump", "col", "nb", "rowsBelow")
        out = self._testSplitRecords(buf, 9, (
            ("levels", n[0], ("panels",) + panel),
            ("items", n[1], ("kind", "slot", "l", "e", "w", "nBlocks", "rowsBelow", "invSlot", "xchgOff", "fwdWgs",
                             "bwdWgs")),
            ("invPanels", n[2], panel)))
        out.update(numSweeps=n[3], sweepInstStride=n[4], maxSweepWgs=n[5], maxSweepWgsM=n[6], maxSweepW=n[7],
                   maxSweepBelow=n[8])
        return out

    def collectOpStats(self, on=True):
        """Solver::enableStats + per-op samples of the per-op boundary (bsp_collect_op_stats)"""
        _check(self._lib.bsp_collect_op_stats(self._h, ctypes.c_int32(1 if on else 0)))

    def opStats(self):
        """{"potrf": (n,2) [n, s], "trsm": (n,3) [n, k, s], "syge": (n,4) [m, n, k, s],
        "asmbl": (n,3) [blockRows, blockCols, s]} collected since collectOpStats(True)"""
        out = {}
        for which, (name, nsz) in enumerate((("potrf", 1), ("trsm", 2), ("syge", 3), ("asmbl", 2))):
            cnt = ctypes.c_int64(0)
            _check(self._lib.bsp_read_op_stats(self._h, ctypes.c_int32(which), None, ctypes.c_int64(0),
                                               ctypes.byref(cnt)))
            buf = np.zeros((cnt.value, 4))
            if cnt.value:
                _check(self._lib.bsp_read_op_stats(
                    self._h, ctypes.c_int32(which), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                    ctypes.c_int64(cnt.value), ctypes.byref(cnt)))
            out[name] = np.concatenate([buf[:, :nsz], buf[:, 3:4]], axis=1)
        return out

    def _factor_partial_batched(self, which, data, span_index):
        for t in data:
            self._check_data(t)
        ptrs = _ptr_array(data)
        _check(getattr(self._lib, "bsp_factor_partial_batched_" + _suffix(data[0]))(
            self._h, ptrs, ctypes.c_int32(len(data)), ctypes.c_int64(span_index), ctypes.c_int32(which)))

    def factorUpTo(self, data, span_index):
        """Solver::factorUpTo<T> / <std::vector<T*>> (list/tuple of tensors = batch)"""
        if isinstance(data, (list, tuple)):
            return self._factor_partial_batched(0, data, span_index)
        self._check_data(data)
        _check(getattr(self._lib, "bsp_factor_up_to_" + _suffix(data))(
            self._h, ctypes.c_void_p(_ptr_of(data)), ctypes.c_int64(span_index)))

    def factorFrom(self, data, span_index):
        if isinstance(data, (list, tuple)):
            return self._factor_partial_batched(1, data, span_index)
        self._check_data(data)
        _check(getattr(self._lib, "bsp_factor_from_" + _suffix(data))(
            self._h, ctypes.c_void_p(_ptr_of(data)), ctypes.c_int64(span_index)))

    def doElimination(self, data, elim_range_index):
        """TESTING hook: numCtx->doElimination(internalGetElimCtx(i), ...)"""
        self._check_data(data)
        _check(getattr(self._lib, "bsp_do_elimination_" + _suffix(data))(
            self._h, ctypes.c_void_p(_ptr_of(data)), ctypes.c_int64(elim_range_index)))

    def _solve(self, name, mat, vec, stride, nrhs):
        if stride is None:
            stride = self.order()
        if isinstance(mat, (list, tuple)):  # batch: one factored matrix and one vector block each
            assert isinstance(vec, (list, tuple)) and len(vec) == len(mat)
            for t in mat:
                self._check_data(t)
            which = {"bsp_solve_": 0, "bsp_solve_l_": 1, "bsp_solve_lt_": 2}[name]
            mats = _ptr_array(mat)
            vecs = _ptr_array(vec)
            _check(getattr(self._lib, "bsp_solve_batched_" + _suffix(mat[0]))(
                self._h, mats, vecs, ctypes.c_int32(len(mat)), ctypes.c_int64(stride),
                ctypes.c_int32(nrhs), ctypes.c_int32(which)))
            return
        self._check_data(mat)
        _check(getattr(self._lib, name + _suffix(mat))(
            self._h, ctypes.c_void_p(_ptr_of(mat)), ctypes.c_void_p(_ptr_of(vec)),
            ctypes.c_int64(stride), ctypes.c_int32(nrhs)))

    def solve(self, mat, vec, stride=None, nRHS=1):
        self._solve("bsp_solve_", mat, vec, stride, nRHS)

    def solveL(self, mat, vec, stride=None, nRHS=1):
        self._solve("bsp_solve_l_", mat, vec, stride, nRHS)

    def solveLt(self, mat, vec, stride=None, nRHS=1):
        self._solve("bsp_solve_lt_", mat, vec, stride, nRHS)

    # ---- products with the factor -----------------------------------------
    def _factor_product(self, what, which, L, x, out, stride, nRHS):
        import torch
        if out is None:
            if isinstance(x, (list, tuple)):
                out = [torch.empty_like(t) for t in x]
            else:
                out = torch.empty_like(x)
        batched, (ls, xs, outs) = self._same_kind(what, "L, x and out", L, x, out)
        for t in ls:
            self._check_data(t)
        if stride is None:
            stride = self.order()
        need = stride * (nRHS - 1) + self.order()
        for t in xs + outs:
            if nRHS >= 1 and t.numel() < need:
                raise ValueError("%s: a vector block of %d elements is too short for nRHS = %d at stride %d"
                                 % (what, t.numel(), nRHS, stride))
        _call(self._lib, "bsp_factor_product_", batched, _suffix(ls[0]), self._h, _ptr_arg(ls, batched),
              ctypes.c_int32(which), _ptr_arg(xs, batched), ctypes.c_int64(stride), _ptr_arg(outs, batched),
              ctypes.c_int64(stride), ctypes.c_int32(nRHS), *_count(outs, batched))
        return out

    def mulL(self, L, x, out=None, stride=None, nRHS=1):
        """extension: out = L x on the device (bsp_factor_product_*, which = 0).  `L`: a buffer in the
        numeric layout, of which only the stored elements i >= j are read (a factor(), or any data); x
        and out: order x nRHS, column-major with leading dimension `stride` (default order()), e.g.
        tensors [nRHS, order], in internal order as for solve().  L and x are only read; every element
        of out is written once, none is read (out=None: a new tensor like x).  Sums run in an order
        fixed by the structure, without atomics: results are bitwise reproducible, column k is bitwise
        the call on that column alone, and lists/tuples of tensors = a batch whose member q is bitwise
        the single call.  Returns out."""
        return self._factor_product("mulL", 0, L, x, out, stride, nRHS)

    def mulLt(self, L, x, out=None, stride=None, nRHS=1):
        """extension: out = L^T x on the device (bsp_factor_product_*, which = 1); arguments as mulL."""
        return self._factor_product("mulLt", 1, L, x, out, stride, nRHS)

    def _solve_partial(self, which, mat, span_index, vec, stride, nrhs):
        if stride is None:
            stride = self.order()
        if isinstance(mat, (list, tuple)):  # batch
            assert isinstance(vec, (list, tuple)) and len(vec) == len(mat)
            for t in mat:
                self._check_data(t)
            mats = _ptr_array(mat)
            vecs = _ptr_array(vec)
            _check(getattr(self._lib, "bsp_solve_partial_batched_" + _suffix(mat[0]))(
                self._h, mats, vecs, ctypes.c_int32(len(mat)), ctypes.c_int64(stride),
                ctypes.c_int32(nrhs), ctypes.c_int32(which), ctypes.c_int64(span_index)))
            return
        self._check_data(mat)
        _check(getattr(self._lib, "bsp_solve_partial_" + _suffix(mat))(
            self._h, ctypes.c_void_p(_ptr_of(mat)), ctypes.c_void_p(_ptr_of(vec)),
            ctypes.c_int64(stride), ctypes.c_int32(nrhs), ctypes.c_int32(which),
            ctypes.c_int64(span_index)))

    def solveLUpTo(self, mat, span_index, vec, stride=None, nRHS=1):
        self._solve_partial(0, mat, span_index, vec, stride, nRHS)

    def solveLtUpTo(self, mat, span_index, vec, stride=None, nRHS=1):
        self._solve_partial(1, mat, span_index, vec, stride, nRHS)

    def solveLFrom(self, mat, span_index, vec, stride=None, nRHS=1):
        self._solve_partial(2, mat, span_index, vec, stride, nRHS)

    def solveLtFrom(self, mat, span_index, vec, stride=None, nRHS=1):
        self._solve_partial(3, mat, span_index, vec, stride, nRHS)

    def addMvFrom(self, mat, span_index, vec_in, in_stride, vec_out, out_stride, nRHS=1, alpha=1.0):
        """Solver::addMvFrom: out += alpha * A * in on the block from span_index on"""
        self._check_data(mat)
        sfx = _suffix(mat)
        a = ctypes.c_double(alpha) if sfx == "f64" else ctypes.c_float(alpha)
        _check(getattr(self._lib, "bsp_add_mv_from_" + sfx)(
            self._h, ctypes.c_void_p(_ptr_of(mat)), ctypes.c_int64(span_index),
            ctypes.c_void_p(_ptr_of(vec_in)), ctypes.c_int64(in_stride),
            ctypes.c_void_p(_ptr_of(vec_out)), ctypes.c_int64(out_stride), ctypes.c_int32(nRHS), a))

    def pseudoFactorFrom(self, data, span_index):
        """Solver::pseudoFactorFrom: per-span diagonal Cholesky + division of the rows below"""
        self._check_data(data)
        _check(getattr(self._lib, "bsp_pseudo_factor_from_" + _suffix(data))(
            self._h, ctypes.c_void_p(_ptr_of(data)), ctypes.c_int64(span_index)))

    def selectedInverse(self, data):
        """extension: selected inversion, in place.  `data` holds a complete factor() of this
        solver; it is overwritten by Z = A^-1 on the block pattern of L, in the factor's layout
        (diagonal blocks full and symmetric, off-diagonal blocks in their stored orientation: the
        accessors read Z as they read L).  bsp_selected_inverse_f64 / _f32.
        A list/tuple of tensors (one dtype, distinct buffers) = a batch of factors of this solver
        (bsp_selected_inverse_batched_*): member q is bitwise selectedInverse(data[q])."""
        batched, (ds,) = self._same_kind("selectedInverse", "data", data)
        for t in ds:
            self._check_data(t)
        _call(self._lib, "bsp_selected_inverse_", batched, _suffix(ds[0]), self._h, _ptr_arg(ds, batched),
              *_count(ds, batched))

    def marginals(self, data, params):
        """diagonal covariance blocks of the given user-order parameters, read from the output of
        selectedInverse(data): a device tensor [k, n, n] when every parameter has size n, else a
        list of [n_i, n_i] tensors.  `data` a list/tuple of B tensors (a batch): [B, k, n, n] when
        every parameter has size n, else one such list per matrix"""
        if isinstance(data, (list, tuple)):
            if len(data) == 0:
                raise ValueError("marginals: empty batch")
            import torch
            per = [self.marginals(t, params) for t in data]
            if all(isinstance(m, torch.Tensor) for m in per):
                return torch.stack(per)
            return per
        params = [int(p) for p in params]
        num = self.numSpans()
        for p in params:
            if p < 0 or p >= num:
                raise IndexError("marginals: parameter %d out of range [0, %d)" % (p, num))
        self._check_data(data)
        import torch
        ss = self.skel()["spanStart"]
        p2s = self.paramToSpan()
        sizes = [int(ss[p2s[p] + 1] - ss[p2s[p]]) for p in params]
        offs = [self.diagBlockOffset(p) for p in params]
        if len(params) == 0:
            return torch.empty((0, 0, 0), dtype=data.dtype, device=data.device)
        if len(set(sizes)) == 1:
            n = sizes[0]
            base = torch.tensor([o for o, _ in offs], dtype=torch.int64)
            stride = torch.tensor([st for _, st in offs], dtype=torch.int64)
            r = torch.arange(n, dtype=torch.int64)
            idx = base[:, None, None] + r[None, :, None] * stride[:, None, None] + r[None, None, :]
            return data[idx.to(data.device)]
        return [data.as_strided((n, n), (st, 1), o).clone() for n, (o, st) in zip(sizes, offs)]

    def logDet(self, data):
        """extension: log det A = 2 sum_i log L_ii of a complete factor() in `data`, accumulated in
        fp64 (bsp_log_det_f64 / _f32).  Returns a 0-dim device tensor of data's dtype, enqueued on the
        solver's stream without synchronising; a non-positive or NaN pivot gives -inf or NaN.  A
        list/tuple of tensors (one dtype) = a batch: a device tensor [B] (bsp_log_det_batched_*)."""
        import torch
        batched, (ds,) = self._same_kind("logDet", "data", data)
        for t in ds:
            self._check_data(t)
        out = torch.empty((len(ds),) if batched else (), dtype=ds[0].dtype, device=ds[0].device)
        _call(self._lib, "bsp_log_det_", batched, _suffix(ds[0]), self._h, _ptr_arg(ds, batched),
              ctypes.c_void_p(_ptr_of(out)), *_count(ds, batched))
        return out

    # ---- status of a factor, damping, regularised retry -----------------
    def _span_range(self, what, spanBegin, spanEnd):
        spanEnd = self.numSpans() if spanEnd is None else int(spanEnd)
        spanBegin = int(spanBegin)
        if not 0 <= spanBegin <= spanEnd <= self.numSpans():
            raise ValueError("%s: the span range [%d, %d) is not inside [0, %d]" % (what, spanBegin, spanEnd,
                                                                                  self.numSpans()))
        return spanBegin, spanEnd

    def _torch_stream(self, device):
        """the stream of setStream() as a torch stream of `device` (None: the default stream)"""
        import torch
        st = self._stream
        if st is None or (isinstance(st, int) and st == 0):
            return torch.cuda.default_stream(device)
        if isinstance(st, int):
            return torch.cuda.ExternalStream(st, device=device)
        return st

    def factorStatus(self, data, spanBegin=0, spanEnd=None):
        """extension: the status record of the stored diagonals of the internal scalars of the spans
        [spanBegin, spanEnd) of `data` (bsp_factor_status_*): a device int64 tensor [4] =
        {lowest bad internal scalar or -1, number of bad diagonals, bits of the float64 minimum over the
        good diagonals (+inf: none), bits of the float64 maximum (0.0: none)}; a diagonal is good when it
        is positive and finite.  `data` is only read.  Enqueued on the solver's stream without
        synchronising: readFactorStatus() decodes it.  After factor() the range is all spans, after
        factorUpTo(span) [0, span), after factorFrom(span) [span, numSpans()); on an unfactored matrix
        the record describes diag(A).  A list/tuple of tensors (one dtype) = a batch: [B, 4], member q
        bitwise the single call.  The record is written on the solver's stream (setStream): a caller
        that reads it with torch on another stream orders the two itself, as for logDet();
        readFactorStatus() waits for the solver's stream."""
        import torch
        b, e = self._span_range("factorStatus", spanBegin, spanEnd)
        batched, (ds,) = self._same_kind("factorStatus", "data", data)
        for t in ds:
            self._check_data(t)
        out = torch.empty((len(ds), 4) if batched else (4,), dtype=torch.int64, device=ds[0].device)
        _call(self._lib, "bsp_factor_status_", batched, _suffix(ds[0]), self._h, _ptr_arg(ds, batched),
              ctypes.c_int64(b), ctypes.c_int64(e), ctypes.c_void_p(_ptr_of(out)), *_count(ds, batched))
        return out

    def readFactorStatus(self, t):
        """the record(s) of factorStatus() decoded on the host (this synchronises: one read of 32 bytes
        per matrix).  A dict {ok, first, param, offsetInParam, count, minDiag, maxDiag}, or a list of
        them for [B, 4]: `first` is the lowest bad internal scalar (-1 when ok), `param` the caller's
        parameter that holds it and `offsetInParam` its place inside it (None when ok), `count` the
        number of bad diagonals, minDiag / maxDiag the range of the good ones (inf / 0.0 without any)."""
        if t.is_cuda:
            self._torch_stream(t.device).synchronize()  # the record is written on the solver's stream
        w = t.detach().cpu().numpy().astype(np.int64)
        if w.ndim not in (1, 2) or w.shape[-1] != 4:
            raise ValueError("readFactorStatus: expected an int64 tensor [4] or [B, 4], got shape %s" % (w.shape,))
        ss = self.skel()["spanStart"]
        if getattr(self, "_span_to_param", None) is None:
            self._span_to_param = np.argsort(self.paramToSpan())  # (host, once: the inverse of paramToSpan())
        span_to_param = self._span_to_param

        def decode(r):
            first, count = int(r[0]), int(r[1])
            mn, mx = (float(x) for x in r[2:4].copy().view(np.float64))
            param = off = None
            if first >= 0:
                span = int(np.searchsorted(ss, first, side="right")) - 1
                param, off = int(span_to_param[span]), first - int(ss[span])
            return {"ok": count == 0, "first": first, "param": param, "offsetInParam": off, "count": count,
                    "minDiag": mn, "maxDiag": mx}

        return decode(w) if w.ndim == 1 else [decode(r) for r in w]

    # ---- error bounds; none of these is differentiable -------------------
    def _col_reduce(self, what, fn, a, b, batched):
        import torch
        ts = [a] if b is None else [a, b]
        for t in ts:
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: expected torch.Tensors, got %s" % (what, type(t).__name__))
            _ptr_of(t)
        batched = bool(batched) or a.dim() == 3
        if b is not None and (b.shape != a.shape or b.dtype != a.dtype or b.device != a.device):
            raise ValueError("%s: the operands differ: %s %s on %s and %s %s on %s" % (
                what, tuple(a.shape), a.dtype, a.device, tuple(b.shape), b.dtype, b.device))
        lo = 1 if batched else 0
        if a.dim() not in (lo + 1, lo + 2):
            raise ValueError("%s: expected %s, got shape %s" % (
                what, "[B, n] or [B, n, q]" if batched else "[n] or [n, q]", tuple(a.shape)))
        if batched and a.shape[0] == 0:
            raise ValueError("%s: empty batch" % what)
        has_q = a.dim() == lo + 2
        n, q = a.shape[lo], (a.shape[-1] if has_q else 1)
        if q < 1:
            raise ValueError("%s: no columns" % what)
        out = torch.empty(tuple(a.shape[:lo]) + ((q,) if has_q else ()), dtype=torch.float64, device=a.device)
        ptrs = [_ptr_arg(t.unbind(0) if batched else [t], batched) for t in ts]
        _call(self._lib, fn, batched, _suffix(a), self._h, *ptrs, ctypes.c_int64(n), ctypes.c_int64(q),
              ctypes.c_void_p(_ptr_of(out)), *_count(a, batched))
        return out

    def maxRatio(self, r, d, batched=False):
        """extension: max_i ratio(|r[i, j]|, d[i, j]) per column as a float64 device tensor (bsp_max_ratio_*):
        r and d [n] -> [], [n, q] -> [q], with a leading B when `batched` (three dimensions always are a
        batch).  ratio is 0 when r == 0 and +inf when d == 0 and r != 0; a NaN in either operand makes the
        column's result NaN.  Computed in double for both precisions, two passes, no atomics; bitwise the
        numpy statement.  Enqueued on the solver's stream; the first call that needs more partials than any
        before on this Solver allocates them, which waits for the device, later ones do not synchronise."""
        return self._col_reduce("maxRatio", "bsp_max_ratio_", r, d, batched)

    def colMax(self, a, batched=False):
        """extension: max_i a[i, j] per column as a float64 device tensor, NaN if any element is, -inf for no
        rows (bsp_col_max_*); shapes as for maxRatio."""
        return self._col_reduce("colMax", "bsp_col_max_", a, None, batched)

    NORM_EST_STOPS = ("none", "order one", "repeated sign vector", "no increase", "pass limit", "same column",
                      "non-finite")

    def invNorm1(self, L, scale=None, return_state=False):
        """extension: an estimate of ||A^-1||_1 for the matrix whose complete factor() is `L`, as a float64
        device tensor [] (a list/tuple of factors = a batch: [B]); with scale = D (a device vector of order()
        values in INTERNAL order, or a list of them) of ||D A^-1 D||_1 (bsp_inv_norm1_*).  Hager's estimator
        in Higham's form: a lower bound, almost always within a factor 3.  A fixed schedule of 10 solve()
        calls with one right-hand side on the solver's stream, nothing read back; the workspace is kept with
        this Solver and allocated by the first call of a size.  return_state=True: (estimate, state), state
        the int64 device record [12] / [B, 12] that readNormEstState() decodes.  A factor that broke down
        gives a non-finite estimate.  Not differentiable."""
        import torch
        what = "invNorm1"
        if scale is None:
            batched, (ls,) = self._same_kind(what, "L", L)
            ds = None
        else:
            batched, (ls, ds) = self._same_kind(what, "L and scale", L, scale)
            for t in ds:
                if t.numel() != self.order():
                    raise ValueError("%s: scale has %d elements, the order is %d" % (what, t.numel(), self.order()))
        for t in ls:
            self._check_data(t)
        sfx, dev, nb = _suffix(ls[0]), ls[0].device, len(ls)
        need = ctypes.c_int64(0)
        _check(getattr(self._lib, "bsp_inv_norm1_work_bytes_" + sfx)(self._h, ctypes.byref(need)))
        # one workspace per Solver, grown to the largest need so far
        work = getattr(self, "_norm_est_work", None)
        if work is None or work.device != dev or work.numel() < need.value * nb + 16:
            work = self._norm_est_work = torch.empty(need.value * nb + 16, dtype=torch.uint8, device=dev)
        wptr = (work.data_ptr() + 15) // 16 * 16
        state = torch.empty((nb, 12) if batched else (12,), dtype=torch.int64, device=dev)
        out = torch.empty((nb,) if batched else (), dtype=torch.float64, device=dev)
        _call(self._lib, "bsp_inv_norm1_", batched, sfx, self._h, _ptr_arg(ls, batched), _ptr_arg(ds, batched),
              ctypes.c_void_p(wptr), ctypes.c_void_p(_ptr_of(state)), ctypes.c_void_p(_ptr_of(out)),
              *_count(ls, batched))
        return (out, state) if return_state else out

    def readNormEstState(self, t):
        """the state record(s) of invNorm1(return_state=True) decoded on the host (this synchronises, like
        readFactorStatus).  A dict {est, j, passes, stop, stopReason, altWon, js, alt}, or a list of them for
        [B, 12]: est the estimate, passes how many vectors were measured (1 .. 5), stop the reason code and
        stopReason its name (NORM_EST_STOPS), altWon whether the alternating vector's value won, js the j
        chosen after every pass (internal scalars), alt the alternating vector's value."""
        if t.is_cuda:
            self._torch_stream(t.device).synchronize()
        w = t.detach().cpu().numpy().astype(np.int64)
        if w.ndim not in (1, 2) or w.shape[-1] != 12:
            raise ValueError("readNormEstState: expected an int64 tensor [12] or [B, 12], got shape %s" % (w.shape,))

        def decode(r):
            f = r.copy().view(np.float64)
            return {"est": float(f[0]), "j": int(r[1]), "passes": int(r[2]), "stop": int(r[3]),
                    "stopReason": self.NORM_EST_STOPS[int(r[3])], "altWon": bool(r[4]),
                    "js": [int(x) for x in r[5:10] if x >= 0], "alt": float(f[10])}

        return decode(w) if w.ndim == 1 else [decode(r) for r in w]

    def dampDiagonal(self, data, alpha, beta, spanBegin=0, spanEnd=None):
        """extension: diagonal <- (diagonal * (1 + alpha)) + beta on the device, in place, over the
        internal scalars of the spans [spanBegin, spanEnd) (bsp_damp_*); every operation is rounded in
        the data's dtype (no fused multiply-add): bitwise the numpy statement on scalars of that dtype.
        alpha and beta are floats or device tensors (0-dim or [1]; [B] for a list/tuple of tensors, one
        pair per member): as tensors they are read on the device, so a loop can chain calls without
        synchronising.  No other element of `data` is touched.  Not differentiable (sparse.hessian's
        damping is).  The pairs are packed into one device array on the solver's stream (setStream),
        where the kernel reads it; alpha / beta tensors produced on another stream are the caller's to
        order before the call, like `data`."""
        import torch
        b, e = self._span_range("dampDiagonal", spanBegin, spanEnd)
        batched, (ds,) = self._same_kind("dampDiagonal", "data", data)
        for t in ds:
            self._check_data(t)
        n, dt, dev = len(ds), ds[0].dtype, ds[0].device
        for name, v in (("alpha", alpha), ("beta", beta)):
            if isinstance(v, torch.Tensor) and (v.device != dev or v.numel() not in (1, n)):
                raise ValueError("dampDiagonal: %s must be a float or a tensor of 1 or %d values on %s, got "
                                 "shape %s on %s" % (name, n, dev, tuple(v.shape), v.device))
        # on the solver's stream: the array is written, read by the kernel and released in stream order
        with torch.cuda.stream(self._torch_stream(dev)):
            cols = [v.detach().to(dt).reshape(-1).expand(n) if isinstance(v, torch.Tensor)
                    else torch.full((n,), float(v), dtype=dt, device=dev) for v in (alpha, beta)]
            ab = torch.stack(cols, dim=1).contiguous()  # [n, 2]: alpha, beta of member q at [2 q], [2 q + 1]
        _call(self._lib, "bsp_damp_", batched, _suffix(ds[0]), self._h, _ptr_arg(ds, batched),
              ctypes.c_int64(b), ctypes.c_int64(e), ctypes.c_void_p(_ptr_of(ab)), *_count(ds, batched))
        return data

    def factorRegularized(self, A, out=None, alpha=0.0, beta0=None, growth=10.0, maxRetries=8):
        """extension: factor() with a status check and a damped retry, all on the device.  `A` (a
        tensor, or a list/tuple = a batch) is never written; the factor goes to `out` (allocated when
        None).  Try 0: out.copy_(A); factor(out); status.  Retry t >= 1: out.copy_(A);
        dampDiagonal(out, alpha, beta0 * growth**(t-1)); factor(out); status.  Each try reads 32 bytes
        per member from the device.  Of a batch only the members that failed are tried again (as a
        smaller batch); a member that passes at try 0 holds exactly what factor() of the list gives.
        beta0=None: 8 * eps(dtype) * maxDiag(A) per member, maxDiag read with factorStatus(A) on the
        UNFACTORED matrix -- the scan only reads diagonals, so there it gives the range of diag(A) (1.0
        stands in when A has no good diagonal; a matrix with a bad diagonal can never factor undamped).
        The copies run on the solver's stream (setStream), in order with the kernels; `A` written on
        another stream is the caller's to order before the call.
        Returns (out, info): info = {retries, alpha, beta, status} of the accepted try (beta = 0.0 and
        alpha = 0.0 at try 0), a list of them for a batch.  Raises FactorizationError, which carries
        the last status, when a member still fails after `maxRetries` retries."""
        import torch
        batched = isinstance(A, (list, tuple))
        if out is None:
            out = [torch.empty_like(a) for a in A] if batched else torch.empty_like(A)
        batched, (As, outs) = self._same_kind("factorRegularized", "A and out", A, out)
        for t in As + outs:
            self._check_data(t)
        n = len(As)
        eps = float(torch.finfo(As[0].dtype).eps)
        if beta0 is None:
            st = self.readFactorStatus(self.factorStatus(list(As)))
            betas0 = [8.0 * eps * (s["maxDiag"] if s["maxDiag"] > 0.0 else 1.0) for s in st]
        else:
            betas0 = [float(beta0)] * n
        infos = [None] * n
        pending = list(range(n))
        for t in range(int(maxRetries) + 1):
            po = [outs[q] for q in pending]
            with torch.cuda.stream(self._torch_stream(As[0].device)):
                for q in pending:
                    outs[q].copy_(As[q])
            betas = [0.0 if t == 0 else betas0[q] * float(growth) ** (t - 1) for q in pending]
            if t > 0:
                dt, dev = po[0].dtype, po[0].device
                self.dampDiagonal(po if batched else po[0], torch.full((len(po),), float(alpha), dtype=dt, device=dev),
                                  torch.tensor(betas, dtype=torch.float64).to(dt).to(dev))
            self.factor(po if batched else po[0])
            sts = self.readFactorStatus(self.factorStatus(po))
            failed = []
            for q, b, s in zip(pending, betas, sts):
                infos[q] = {"retries": t, "alpha": float(alpha) if t else 0.0, "beta": b, "status": s}
                if not s["ok"]:
                    failed.append(q)
            pending = failed
            if not pending:
                return out, (infos if batched else infos[0])
        q = pending[0]
        raise FactorizationError(
            "factorRegularized: %s not positive definite after %d retries (last beta %g): the first bad pivot is "
            "internal scalar %d (param %s, offset %s), %d bad diagonals"
            % ("batch member %d is" % q if batched else "the matrix is", int(maxRetries), infos[q]["beta"],
               infos[q]["status"]["first"], infos[q]["status"]["param"], infos[q]["status"]["offsetInParam"],
               infos[q]["status"]["count"]),
            infos[q]["status"], infos if batched else infos[0])

    def patternGrad(self, out, Z=None, zScale=None, U=None, V=None, nRHS=1, alpha=1.0, stride=None):
        """extension: the write-only gradient projection on the pattern of L (bsp_pattern_grad_*).
        For every stored element e = (i, j) of `out` (never read):
          i > j: s 2 Z_e + alpha sum_k (U_ik V_jk + V_ik U_jk);  i = j: s Z_e + alpha sum_k U_ik V_ik;
          strictly-upper elements of the diagonal blocks: 0.
        s = zScale[0], a device tensor (no Z: no first term); U, V column-major order x nRHS with
        leading dimension `stride` (default order()), e.g. tensors [nRHS, order] (none: no second
        term).  `out` a list/tuple = a batch: Z, U, V lists of the same length (or None), s =
        zScale[q] for member q."""
        given = {n: x for n, x in (("out", out), ("Z", Z), ("U", U), ("V", V)) if x is not None}
        batched, ms = self._same_kind("patternGrad", " / ".join(given), *given.values())
        ms = dict(zip(given, ms))
        outs, zs, us, vs = ms["out"], ms.get("Z"), ms.get("U"), ms.get("V")
        if zScale is not None and zScale.dtype != outs[0].dtype:
            raise TypeError("patternGrad: zScale must have the dtype of out (%s), got %s" % (outs[0].dtype, zScale.dtype))
        for t in outs + (zs or []):
            self._check_data(t)
        sfx = _suffix(outs[0])
        real = ctypes.c_double if sfx == "f64" else ctypes.c_float
        _call(self._lib, "bsp_pattern_grad_", batched, sfx, self._h, _ptr_arg(zs, batched),
              ctypes.c_void_p(_ptr_of(zScale) if zScale is not None else None), _ptr_arg(us, batched),
              _ptr_arg(vs, batched), ctypes.c_int64(self.order() if stride is None else stride), ctypes.c_int32(nRHS),
              real(alpha), _ptr_arg(outs, batched), *_count(outs, batched))

    def patternOuter(self, out, U, V, nRHS=1, alpha=1.0, stride=None):
        """extension: the non-symmetric rank-k projection on the pattern of L (bsp_pattern_outer_*).
        For every stored element e = (i, j) of `out` (never read): i >= j: alpha sum_k U_ik V_jk;
        strictly-upper elements of the diagonal blocks: 0.  U, V column-major order x nRHS with leading
        dimension `stride` (default order()), e.g. tensors [nRHS, order].  `out` a list/tuple = a batch:
        U, V lists of the same length."""
        batched, (outs, us, vs) = self._same_kind("patternOuter", "out / U / V", out, U, V)
        for t in outs:
            self._check_data(t)
        sfx = _suffix(outs[0])
        real = ctypes.c_double if sfx == "f64" else ctypes.c_float
        _call(self._lib, "bsp_pattern_outer_", batched, sfx, self._h, _ptr_arg(us, batched), _ptr_arg(vs, batched),
              ctypes.c_int64(self.order() if stride is None else stride), ctypes.c_int32(nRHS), real(alpha),
              _ptr_arg(outs, batched), *_count(outs, batched))

    def factorAdjoint(self, L, grad):
        """extension: the reverse-mode sweep of factor(), in place in `grad` (bsp_factor_adjoint_*).
        `L` holds a complete factor() of A(d) and is only read; `grad` holds df/dL on entry (stored
        elements with i >= j; the strictly-upper elements of the diagonal blocks are ignored) and df/dd
        on return: G_ij + G_ji below the diagonal, G_ii on it, 0 above it.
        Lists/tuples of tensors (one dtype, distinct buffers) = a batch: member q is bitwise the single
        call."""
        batched, (ls, gs) = self._same_kind("factorAdjoint", "L and grad", L, grad)
        for t in ls + gs:
            self._check_data(t)
        _call(self._lib, "bsp_factor_adjoint_", batched, _suffix(gs[0]), self._h, _ptr_arg(ls, batched),
              _ptr_arg(gs, batched), *_count(gs, batched))

    def selectedInverseAdjoint(self, L, Z, grad):
        """extension: the reverse mode of selectedInverse(), in place in `grad`
        (bsp_selected_inverse_adjoint_*).  `L` holds a complete factor(), `Z` what selectedInverse wrote
        over a copy of it; both are only read.  `grad` holds df/d(slot) on entry for EVERY slot of the
        layout as selectedInverse writes it (the strictly-upper elements of the diagonal blocks are slots
        of their own) and Lbar = df/dL on return: the elements i >= j, exactly 0 above the diagonal, the
        input of factorAdjoint.  Lists/tuples of tensors (one dtype, distinct
        gradient buffers) = a batch.  The sweep adds with float atomics: results are close, not bitwise,
        from run to run, and a batch member is close to, not bitwise, the single call."""
        batched, (ls, zs, gs) = self._same_kind("selectedInverseAdjoint", "L, Z and grad", L, Z, grad)
        for t in ls + zs + gs:
            self._check_data(t)
        _call(self._lib, "bsp_selected_inverse_adjoint_", batched, _suffix(gs[0]), self._h, _ptr_arg(ls, batched),
              _ptr_arg(zs, batched), _ptr_arg(gs, batched), *_count(gs, batched))

    # ---- blocks of A^-1 anywhere, by reach solves -----------------------
    INVERSE_BLOCKS_MAX_COLUMNS = 512  # most columns of the distinct params of one bsp_inverse_blocks_* call

    def _param_sizes(self, what, params):
        params = [int(p) for p in params]
        num = self.numSpans()
        for p in params:
            if p < 0 or p >= num:
                raise IndexError("%s: parameter %d out of range [0, %d)" % (what, p, num))
        ss, p2s = self.skel()["spanStart"], self.paramToSpan()
        return params, [int(ss[p2s[p] + 1] - ss[p2s[p]]) for p in params]

    def _reach_out(self, what, L, out, numel, shape):
        """the output of a reach operation: a fresh tensor, or the caller's contiguous `out` of numel elements"""
        import torch
        if out is None:
            return torch.empty(shape, dtype=L.dtype, device=L.device)
        if out.dtype != L.dtype or out.device != L.device or out.numel() != numel or not out.is_contiguous():
            raise ValueError("%s: out must be a contiguous %s tensor of %d elements on %s" % (what, L.dtype, numel,
                                                                                          L.device))
        return out.view(shape)

    def halfInverseColumns(self, L, params, out=None):
        """extension: W = L^-1 E for the unit columns E of the caller's params, stacked in the order
        given: a device tensor [m, order()] (row c = column c of L^-1 E, in internal order).  `L` holds a
        complete factor() and is only read.  Only the lumps on each column's reach are visited
        (bsp_reach_solve_l_*); enqueued on the solver's stream.  out: a contiguous
        tensor of m * order() elements to write instead of a fresh one."""
        self._check_data(L)
        params, sizes = self._param_sizes("halfInverseColumns", params)
        W = self._reach_out("halfInverseColumns", L, out, sum(sizes) * self.order(), (sum(sizes), self.order()))
        if W.numel() == 0:
            return W
        prm = _i64(params)
        _check(getattr(self._lib, "bsp_reach_solve_l_" + _suffix(L))(
            self._h, ctypes.c_void_p(_ptr_of(L)), ctypes.c_int64(len(params)), prm.ctypes.data_as(_I64P),
            ctypes.c_void_p(_ptr_of(W))))
        return W

    def inverseColumns(self, L, params):
        """extension: the columns of A^-1 of the caller's params, stacked in the order given: a device
        tensor [m, order()], rows of A^-1 in internal order (halfInverseColumns, then solveLt)."""
        X = self.halfInverseColumns(L, params)
        if X.shape[0] > 0:
            self.solveLt(L, X, stride=self.order(), nRHS=X.shape[0])
        return X

    def inverseBlocks(self, L, pairs, out=None):
        """extension: the blocks A^-1[P, Q] of the pairs (P, Q) of caller's params, on or off the block
        pattern of L: a device tensor [K, n, n] when every block has one shape, else a list of [n_P, n_Q]
        tensors.  `L` holds a complete factor() and is only read (bsp_inverse_blocks_*; DESIGN.md section
        20).  The pairs run in chunks whose distinct params hold at most INVERSE_BLOCKS_MAX_COLUMNS (512)
        columns (a single pair may exceed it), which bounds the solver's workspace at 512 x order()
        values.  Enqueued on the solver's stream; bitwise reproducible.  out: a contiguous tensor that
        holds the blocks one after the other, to write instead of a fresh one."""
        self._check_data(L)
        pairs = [(int(p), int(q)) for p, q in pairs]
        _, rs = self._param_sizes("inverseBlocks", [p for p, _ in pairs])
        _, cs = self._param_sizes("inverseBlocks", [q for _, q in pairs])
        offs = np.zeros(len(pairs) + 1, dtype=np.int64)
        np.cumsum([a * b for a, b in zip(rs, cs)], out=offs[1:])
        out = self._reach_out("inverseBlocks", L, out, int(offs[-1]), (int(offs[-1]),))
        fn = getattr(self._lib, "bsp_inverse_blocks_" + _suffix(L))
        k0 = 0
        while k0 < len(pairs):
            seen, cols, k1 = set(), 0, k0
            while k1 < len(pairs):
                add = sum(w for prm, w in {pairs[k1][0]: rs[k1], pairs[k1][1]: cs[k1]}.items() if prm not in seen)
                if k1 > k0 and cols + add > self.INVERSE_BLOCKS_MAX_COLUMNS:
                    break
                seen.update(pairs[k1])
                cols += add
                k1 += 1
            rp, cp = _i64([p for p, _ in pairs[k0:k1]]), _i64([q for _, q in pairs[k0:k1]])
            o = np.ascontiguousarray(offs[k0:k1 + 1])
            _check(fn(self._h, ctypes.c_void_p(_ptr_of(L)), ctypes.c_int64(k1 - k0), rp.ctypes.data_as(_I64P),
                      cp.ctypes.data_as(_I64P), ctypes.c_void_p(_ptr_of(out)), o.ctypes.data_as(_I64P)))
            k0 = k1
        if len(pairs) > 0 and len(set(zip(rs, cs))) == 1:
            return out.view(len(pairs), rs[0], cs[0])
        return [out[int(offs[k]):int(offs[k + 1])].view(rs[k], cs[k]) for k in range(len(pairs))]

    def jointMarginal(self, L, params):
        """extension: the dense symmetric covariance [m, m] of the stacked caller's params, A^-1 on their
        rows and columns: the blocks (P, Q) with P at or behind Q in `params` from inverseBlocks, mirrored
        (symmetric to the last bit)."""
        import torch
        params, sizes = self._param_sizes("jointMarginal", params)
        start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pairs = [(i, j) for i in range(len(params)) for j in range(i + 1)]
        blocks = self.inverseBlocks(L, [(params[i], params[j]) for i, j in pairs])
        C = torch.empty((int(start[-1]), int(start[-1])), dtype=L.dtype, device=L.device)
        for (i, j), b in zip(pairs, blocks):
            C[start[i]:start[i + 1], start[j]:start[j + 1]] = b
            if i != j:
                C[start[j]:start[j + 1], start[i]:start[i + 1]] = b.t()
        return C

    # ---- arguments that are one tensor each, or lists of tensors = a batch ---------------------
    def _same_kind(self, what, names, *xs):
        """(batched, [members of every x]) for arguments that are all tensors or all lists of one length"""
        kinds = {isinstance(x, (list, tuple)) for x in xs}
        if len(kinds) != 1:
            raise TypeError("%s: %s must all be tensors or all be lists" % (what, names))
        batched = kinds.pop()
        ms = [list(x) if batched else [x] for x in xs]
        if len(ms[0]) == 0:
            raise ValueError("%s: empty batch" % what)
        if len({len(m) for m in ms}) != 1:
            raise ValueError("%s: %s have %s members" % (what, names, " / ".join(str(len(m)) for m in ms)))
        ts = [t for m in ms for t in m]
        if len({t.dtype for t in ts}) != 1:
            raise TypeError("%s: every tensor must share one dtype, got %s" % (what, sorted({str(t.dtype) for t in ts})))
        if len({t.device for t in ts}) != 1:
            raise ValueError("%s: tensors on different devices: %s" % (what, sorted({str(t.device) for t in ts})))
        return batched, ms

    # ---- the partial factor and its Schur complement -----------------
    def _schurOrder(self, span):
        """scalars from span `span` on: the order m of the Schur complement of factorUpTo(span)"""
        if not 0 <= span <= self.numSpans():
            raise ValueError("span %d is not in [0, %d]" % (span, self.numSpans()))
        return self.order() - int(self.skel()["spanStart"][span])

    def factorAdjointUpTo(self, P, grad, span):
        """extension: the reverse-mode sweep of factorUpTo(span), in place in `grad`
        (bsp_factor_adjoint_up_to_*).  `P` holds factorUpTo(span) of A(d) -- L11, L21 before the cut, the
        Schur complement S behind it -- and is only read; `grad` holds df/dP on entry (stored elements
        with i >= j; strictly-upper elements ignored) and df/dd on return.
        span = numSpans() is factorAdjoint.  Lists/tuples = a batch, member q bitwise the single call."""
        batched, (ps, gs) = self._same_kind("factorAdjointUpTo", "P and grad", P, grad)
        for t in ps + gs:
            self._check_data(t)
        _call(self._lib, "bsp_factor_adjoint_up_to_", batched, _suffix(gs[0]), self._h, _ptr_arg(ps, batched),
              _ptr_arg(gs, batched), *_count(gs, batched), ctypes.c_int64(span))

    def _schur_dense(self, what, name, src, span, out, dest, to_dense):
        import torch
        m = self._schurOrder(span)
        batched = isinstance(src, (list, tuple))
        srcs = list(src) if batched else [src]
        if len(srcs) == 0:
            raise ValueError("%s: empty batch" % what)
        dense_shape, n_dense, n_data = (m, m), m * m, self.dataSize()
        if out is None:
            outs = [torch.empty(dense_shape if to_dense else (n_data,), dtype=t.dtype, device=t.device) for t in srcs]
            out = outs if batched else outs[0]
        batched, (srcs, outs) = self._same_kind(what, "%s and out" % name, src, out)
        for t in srcs:
            if t.numel() != (n_data if to_dense else n_dense):
                raise ValueError("%s: %s has %d elements, expected %d" % (
                    what, name, t.numel(), n_data if to_dense else n_dense))
        for t in outs:
            if t.numel() != (n_dense if to_dense else n_data):
                raise ValueError("%s: out has %d elements, expected %d" % (
                    what, t.numel(), n_dense if to_dense else n_data))
        dp = None
        if dest is not None:
            if dest.dtype != torch.int32 or dest.numel() != m or dest.device != srcs[0].device:
                raise ValueError("%s: dest must be an int32 tensor of %d elements on %s" % (what, m, srcs[0].device))
            dp = _ptr_of(dest)
        _call(self._lib, "bsp_schur_to_dense_" if to_dense else "bsp_schur_from_dense_", batched, _suffix(srcs[0]),
              self._h, _ptr_arg(srcs, batched), ctypes.c_int64(span), _ptr_arg(outs, batched), ctypes.c_void_p(dp),
              *_count(outs, batched))
        return out

    def schurComplement(self, P, span, out=None, dest=None):
        """extension: the trailing block of the layout buffer `P` (e.g. after factorUpTo(span): the Schur
        complement) as a dense symmetric [m, m] tensor, m = order() - spanStart[span] (bsp_schur_to_dense_*): row /
        column dest[k] for the k-th scalar behind the cut (`dest`: int32 device permutation; None =
        internal order), zeros where the pattern has no block.  Every element of `out` is written (it
        is allocated when None).  Lists = a batch.  Returns out."""
        return self._schur_dense("schurComplement", "P", P, span, out, dest, True)

    def schurComplementAdjoint(self, gradDense, span, out=None, dest=None):
        """extension: the adjoint of schurComplement (bsp_schur_from_dense_*): a gradient in the data
        layout from a dense [m, m] gradient (it need not be symmetric): g_ij + g_ji below the diagonal of
        the trailing block, g_ii on it, 0 above it and on every column before the cut.  Every element of
        `out` ([dataSize], allocated when None) is written.  Lists = a batch.  Returns out."""
        return self._schur_dense("schurComplementAdjoint", "gradDense", gradDense, span, out, dest, False)

    # ---- assembly of coordinate entries -----------------------------
    def assembly(self, rows, cols, triangle="lower"):
        """extension: the map from coordinate entries (rows[k], cols[k]) in the caller's scalar order to
        this solver's layout (bsp_assembly_create), built once on the host.  triangle "lower": every
        entry has row >= col; "full": entries with row < col are skipped.  See Assembly."""
        return Assembly(self, rows, cols, triangle)

    # ---- normal equations of a sparse Jacobian -----------------------
    def normalEquations(self, rows, cols, m):
        """extension: the maps from the entries (rows[k], cols[k]) of an m x order() Jacobian in the
        caller's scalar order to this solver's layout (bsp_normal_eq_create), built once on the host.
        No (row, col) may repeat.  See NormalEquations."""
        return NormalEquations(self, rows, cols, m)

    # ---- products with a matrix given as entries ---------------------
    def symProduct(self, rows, cols, triangle="lower"):
        """extension: the map of the products with the symmetric matrix of the coordinate entries
        (rows[k], cols[k]) in the caller's scalar order (bsp_sym_product_create), built once on the
        host; triangle as for assembly().  See SymProduct."""
        return SymProduct(self, rows, cols, triangle)

    # ---- products with a Jacobian given as entries ---------------------
    def jacobianProduct(self, rows, cols, m):
        """extension: the map of the products with the m x order() Jacobian of the entries (rows[k], cols[k])
        in the caller's scalar order (bsp_jac_product_create), built once on the host; this solver's layout
        is never touched.  No (row, col) may repeat.  See JacobianProduct."""
        return JacobianProduct(self, rows, cols, m)

    def jacobianSchur(self, product, eliminate):
        """extension: the map of the implicit Schur elimination of the params `eliminate` (indices into this
        solver's params) on the JacobianProduct `product` (bsp_jac_schur_create), built once on the host.  See
        JacobianSchur."""
        if not isinstance(product, JacobianProduct) or product.solver is not self:
            raise ValueError("jacobianSchur: product must be a JacobianProduct of this solver")
        return JacobianSchur(product, eliminate)

    def diagOffsets(self):
        """extension: int64 array [order()], the layout offsets of the diagonal elements in internal
        order (what damp() touches)"""
        sk = self.skel()
        ls = sk["lumpStart"]
        w = (ls[1:] - ls[:-1]).astype(np.int64)
        d0 = sk["chainData"][sk["chainColPtr"][:-1]].astype(np.int64)
        local = np.arange(self.order(), dtype=np.int64) - np.repeat(ls[:-1], w)
        return np.repeat(d0, w) + local * (np.repeat(w, w) + 1)

    def scalarPermutation(self):
        """extension: int64 array p of length order(), p[i_user] = i_internal (bsp_scalar_permutation)"""
        out = np.empty(self.order(), dtype=np.int64)
        _check(self._lib.bsp_scalar_permutation(self._h, out.ctypes.data_as(_I64P)))
        return out

    # ---- measurement --------------------------------------------------------------------
    def factorFlops(self):
        return float(self._lib.bsp_factor_flops(self._h))

    def planLevels(self):
        """level table of the factor plan (bsp_plan_levels): int64 array [levels, 8]"""
        self._lib.bsp_plan_levels.restype = ctypes.c_int64
        n = self._lib.bsp_plan_levels(self._h, None, ctypes.c_int64(0))
        if n < 0:
            raise RuntimeError(_lib.load().bsp_last_error().decode("utf-8", "replace"))
        out = np.zeros(n, dtype=np.int64)
        self._lib.bsp_plan_levels(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_int64(n))
        return out.reshape(-1, 8)

    def planStats(self):
        st = _CPlanStats()
        _check(self._lib.bsp_plan_stats_full(self._h, ctypes.byref(st)))
        return {n: getattr(st, n) for n, _ in _CPlanStats._fields_}

    def runCounters(self):
        """what the calls on this solver actually ran (bsp_run_counters_get): persistent sweeps
        launched / timed out, split-K lists used, sub-batches enqueued, lookahead forks"""
        st = _CRunCounters()
        _check(self._lib.bsp_run_counters_get(self._h, ctypes.byref(st)))
        # (gather_chunks_overlapped only keeps the layout of bsp_run_counters: always 0)
        return {n: getattr(st, n) for n, _ in _CRunCounters._fields_ if n != "gather_chunks_overlapped"}

    def factorProfiled(self, data, in_situ=False, busy=False):
        """one factor() with every launch bracketed by HIP events; returns {kernel class: (total
        ms, launches)}.  in_situ=False: launches serialised on the execution stream (isolated
        kernel times); in_situ=True: the real two-stream schedule, each launch timed on the stream
        it runs on; busy=True adds, per class, the time during which at least one of its launches
        was running (launches on different streams overlap)"""
        self._check_data(data)
        ms = (ctypes.c_double * 6)()
        ln = (ctypes.c_int64 * 6)()
        if in_situ and busy:
            bs = (ctypes.c_double * 6)()
            _check(self._lib.bsp_factor_profiled_busy_f64(self._h, ctypes.c_void_p(_ptr_of(data)), ms, ln, bs))
            return {k: (ms[i], ln[i], bs[i]) for i, k in enumerate(PROF_KINDS)}
        fn = self._lib.bsp_factor_profiled_insitu_f64 if in_situ else self._lib.bsp_factor_profiled_f64
        _check(fn(self._h, ctypes.c_void_p(_ptr_of(data)), ms, ln))
        return {k: (ms[i], ln[i]) for i, k in enumerate(PROF_KINDS)}

    # ---- host helpers on the skeleton (CoalescedBlockMatrix.cpp:124-187) ------------------
    def densify(self, data, fill_upper_half=False, start_span_index=0):
        """dense numpy copy of host `data` laid out by this solver's skeleton"""
        sk = self.skel()
        data = np.asarray(data)
        off = int(sk["spanStart"][start_span_index])
        n = self.order() - off
        dense = np.zeros((n, n), dtype=data.dtype)
        ls, ss = sk["lumpStart"], sk["spanStart"]
        for l in range(int(sk["spanToLump"][start_span_index]), self.numLumps()):
            w = int(ls[l + 1] - ls[l])
            for c in range(int(sk["chainColPtr"][l]), int(sk["chainColPtr"][l + 1])):
                sp = int(sk["chainRowSpan"][c])
                r0, rows = int(ss[sp]) - off, int(ss[sp + 1] - ss[sp])
                d0 = int(sk["chainData"][c])
                dense[r0:r0 + rows, int(ls[l]) - off:int(ls[l]) - off + w] = \
                    data[d0:d0 + rows * w].reshape(rows, w)
        if fill_upper_half:
            dense = np.tril(dense) + np.tril(dense, -1).T
        return dense

    def lowerMask(self):
        """boolean mask over the numeric data: False on the strictly-upper entries of the square
        diagonal blocks (stored but meaningless, CoalescedBlockMatrix.h:23-37), True elsewhere"""
        sk = self.skel()
        ls = sk["lumpStart"]
        w = (ls[1:] - ls[:-1]).astype(np.int64)
        d0 = sk["chainData"][sk["chainColPtr"][:-1]]
        mask = np.ones(self.dataSize(), dtype=bool)
        for width in np.unique(w):
            if width < 2:
                continue
            i, j = np.triu_indices(int(width), 1)
            upper = (i * width + j).astype(np.int64)
            starts = d0[w == width]
            mask[(starts[:, None] + upper[None, :]).ravel()] = False
        return mask

    def damp(self, data, alpha, beta):
        """diagonal <- diagonal * (1 + alpha) + beta, in place on a host numpy array"""
        sk = self.skel()
        ls = sk["lumpStart"]
        w = (ls[1:] - ls[:-1]).astype(np.int64)
        d0 = sk["chainData"][sk["chainColPtr"][:-1]]
        idx = np.concatenate([d0[i] + np.arange(w[i]) * (w[i] + 1) for i in range(len(w))])
        data[idx] = data[idx] * (1 + alpha) + beta
        return data


_TRIANGLES = {"lower": 0, "full": 1}


def _host_indices(a, name):
    """int64 numpy copy of an index array (numpy, sequence or torch tensor on any device)"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 1:
        raise ValueError("assembly: %s must be one-dimensional, got shape %s" % (name, a.shape))
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError("assembly: %s must hold integers, got %s" % (name, a.dtype))
    return _i64(a)


class _EntryMap:
    """what Assembly, NormalEquations and SymProduct share: the handle of the host map that
    bsp_<_C>_create builds from (rows, cols), its figures, and the tail of every device call"""
    _C = None    # the map's C entries are bsp_<_C>_create, bsp_<_C>_destroy and bsp_<_C>_info
    _KEYS = ()   # the figures of bsp_<_C>_info, in its order

    def _create(self, op, solver, rows, cols, before=(), after=()):
        """builds the map; `before` / `after`: the C arguments before nnz and behind cols"""
        self._lib = solver._lib
        self._h = None
        r, c = _host_indices(rows, "rows"), _host_indices(cols, "cols")
        if len(r) != len(c):
            raise ValueError("%s: %d rows for %d cols" % (op, len(r), len(c)))
        h = ctypes.c_void_p()
        _check(getattr(self._lib, "bsp_%s_create" % self._C)(
            solver._h, *before, ctypes.c_int64(len(r)), r.ctypes.data_as(_I64P), c.ctypes.data_as(_I64P), *after,
            ctypes.byref(h)))
        self._h = h
        self.solver = solver
        self.nnz = len(r)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            getattr(self._lib, "bsp_%s_destroy" % self._C)(h)

    def info(self):
        """figures of the map (bsp_<_C>_info)"""
        out = (ctypes.c_int64 * len(self._KEYS))()
        _check(getattr(self._lib, "bsp_%s_info" % self._C)(self._h, out))
        return dict(zip(self._KEYS, [int(x) for x in out]))

    @staticmethod
    def _alloc_out(name, ref, shape, out):
        """`out` allocated like `ref` with `shape`, or checked against them"""
        import torch
        shape = tuple(shape)
        if out is None:
            return torch.empty(shape, dtype=ref.dtype, device=ref.device)
        if tuple(out.shape) != shape or out.dtype != ref.dtype or out.device != ref.device:
            raise ValueError("%s: out must be %s %s on %s, got %s %s on %s" % (
                name, shape, ref.dtype, ref.device, tuple(out.shape), out.dtype, out.device))
        return out

    def _launch(self, name, fn, sfx, ins, shape, out, batched, q=None):
        """the tail of an operation on the device tensors `ins`: `out` allocated or checked against `shape`,
        every tensor in device memory and contiguous, then the single or the batched entry `fn`"""
        out = self._alloc_out(name, ins[0], shape, out)
        ts = list(ins) + [out]
        for t in ts:
            _ptr_of(t)  # device memory, contiguous
        ptrs = [_ptr_arg(t.unbind(0) if batched else [t], batched) for t in ts]
        qa = [] if q is None else [ctypes.c_int64(q)]
        _call(self._lib, fn, batched, sfx, self.solver._h, self._h, *ptrs[:-1], *qa, ptrs[-1], *_count(out, batched))
        return out


class Assembly(_EntryMap):
    """extension: the host map from coordinate entries (rows[k], cols[k]) in the
    caller's scalar order to a Solver's numeric layout, and the device kernels that use it.  Built by
    Solver.assembly(); keeps its solver alive.  A_ij = A_ji = sum of the values of the entries at
    (i, j), i >= j; duplicates are summed in ascending entry index (bitwise np.add.at).  The first
    assemble / adjoint call uploads the map to the device; both run on the solver's stream without
    synchronising."""

    _C = "assembly"
    _KEYS = ("nnz", "kept", "elements", "max_run", "long_runs", "tiles", "device_bytes")

    def __init__(self, solver, rows, cols, triangle="lower"):
        if triangle not in _TRIANGLES:
            raise ValueError("assembly: triangle must be 'lower' or 'full', got %r" % (triangle,))
        self._create("assembly", solver, rows, cols, after=(ctypes.c_int32(_TRIANGLES[triangle]),))
        self.triangle = triangle

    def entryOffsets(self):
        """int64 array [nnz]: the layout offset of every entry, -1 for a skipped one"""
        out = np.empty(self.nnz, dtype=np.int64)
        _check(self._lib.bsp_assembly_entry_offsets(self._h, out.ctypes.data_as(_I64P)))
        return out

    def _run(self, name, x, n_in, n_out, out, adjoint):
        import torch
        if not isinstance(x, torch.Tensor):
            raise TypeError("%s: expected a torch.Tensor, got %s" % (name, type(x).__name__))
        if x.dim() not in (1, 2) or x.shape[-1] != n_in:
            raise ValueError("%s: expected [%d] or [B, %d], got shape %s" % (name, n_in, n_in, tuple(x.shape)))
        if x.dim() == 2 and x.shape[0] == 0:
            raise ValueError("%s: empty batch" % name)
        return self._launch(name, "bsp_assemble_adjoint_" if adjoint else "bsp_assemble_", _suffix(x), [x],
                            x.shape[:-1] + (n_out,), out, x.dim() == 2)

    def assemble(self, values, out=None):
        """values [nnz] or [B, nnz] (device, float64 / float32) -> the layout [dataSize] / [B, dataSize]:
        every element written, 0 where no entry maps (bsp_assemble_*)"""
        return self._run("assemble", values, self.nnz, self.solver.dataSize(), out, False)

    def adjoint(self, gradData, out=None):
        """gradData [dataSize] or [B, dataSize] -> [nnz] / [B, nnz]: gradData[entryOffsets()], 0 for
        skipped entries (bsp_assemble_adjoint_*)"""
        return self._run("adjoint", gradData, self.solver.dataSize(), self.nnz, out, True)


_I32P = ctypes.POINTER(ctypes.c_int32)


class NormalEquations(_EntryMap):
    """extension: the host maps from the entries (rows[k], cols[k]) of an m x n
    Jacobian J (n = the solver's order(), caller's scalar order, no position repeated) to the solver's
    layout, and the device kernels that use them.  Built by Solver.normalEquations(); keeps its solver
    alive.  hessian: H = J^T J in the layout; hessianAdjoint: the gradient of the values from the gradient
    of the data; jtVec: J^T r; jVec: J v.  Sums run in a fixed order with every product rounded first
    (bitwise the numpy restatement); each part of the map is uploaded by the first call that needs it;
    everything runs on the solver's stream without synchronising."""

    _C = "normal_eq"
    _KEYS = ("nnz", "pairs", "destinations", "max_run", "long_runs", "tiles", "forward_bytes", "adjoint_bytes",
             "vector_bytes", "adjoint_terms")

    def __init__(self, solver, rows, cols, m):
        self._create("normalEquations", solver, rows, cols, before=(ctypes.c_int64(int(m)),))
        self.m = int(m)
        self.n = solver.order()

    def pairTable(self):
        """(ka, kb, offset) of every pair in run order: int32, int32, int64 arrays of info()["pairs"]"""
        P = self.info()["pairs"]
        ka, kb, off = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int64)
        _check(self._lib.bsp_normal_eq_pair_table(self._h, ka.ctypes.data_as(_I32P), kb.ctypes.data_as(_I32P),
                                                  off.ctypes.data_as(_I64P)))
        return ka, kb, off

    def _run(self, name, fn, values, x, x_rows, out_rows, out):
        """values [nnz] / [B, nnz]; x None, or [.., x_rows] / [.., x_rows, q]; out [.., out_rows(, q)]"""
        import torch
        for what, t in (("values", values), (name + " input", x)):
            if t is not None and not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a torch.Tensor, got %s" % (name, what, type(t).__name__))
        if values.dim() not in (1, 2) or values.shape[-1] != self.nnz:
            raise ValueError("%s: values must be [%d] or [B, %d], got shape %s"
                             % (name, self.nnz, self.nnz, tuple(values.shape)))
        batched = values.dim() == 2
        if batched and values.shape[0] == 0:
            raise ValueError("%s: empty batch" % name)
        sfx = _suffix(values)
        lead = tuple(values.shape[:-1])
        q = None
        if x is None:
            shape = lead + (out_rows,)
        else:
            if x.dtype != values.dtype or x.device != values.device:
                raise TypeError("%s: the input is %s on %s, values are %s on %s"
                                % (name, x.dtype, x.device, values.dtype, values.device))
            vec = fn.startswith(("bsp_normal_eq_j", "bsp_jac_product_j"))
            ok = x.dim() in ((len(lead) + 1, len(lead) + 2) if vec else (len(lead) + 1,))
            if not ok or tuple(x.shape[:len(lead)]) != lead or x.shape[len(lead)] != x_rows:
                raise ValueError("%s: the input must be %s%s with leading size %d, got shape %s" % (
                    name, "[B, ...] " if batched else "", "[rows] or [rows, q]" if vec else "[dataSize]", x_rows,
                    tuple(x.shape)))
            if vec:
                q = x.shape[-1] if x.dim() == len(lead) + 2 else 1
                if q < 1:
                    raise ValueError("%s: the input has no vectors" % name)
                shape = lead + (out_rows,) + ((q,) if x.dim() == len(lead) + 2 else ())
            else:
                shape = lead + (out_rows,)
        return self._launch(name, fn, sfx, [values] if x is None else [values, x], shape, out, batched, q)

    def hessian(self, values, out=None):
        """values [nnz] or [B, nnz] (device, float64 / float32) -> H = J^T J in the layout, [dataSize] /
        [B, dataSize]: every element written, 0 where no pair lands (bsp_normal_eq_hessian_*)"""
        return self._run("hessian", "bsp_normal_eq_hessian_", values, None, 0, self.solver.dataSize(), out)

    def hessianAdjoint(self, values, gradData, out=None):
        """gradData [dataSize] or [B, dataSize] -> the gradient of values, [nnz] / [B, nnz]
        (bsp_normal_eq_hessian_adjoint_*)"""
        return self._run("hessianAdjoint", "bsp_normal_eq_hessian_adjoint_", values, gradData,
                         self.solver.dataSize(), self.nnz, out)

    def jtVec(self, values, r, out=None):
        """r [m] or [m, q] (leading B when values are batched) -> J^T r, [n] / [n, q], caller's order
        (bsp_normal_eq_jt_vec_*)"""
        return self._run("jtVec", "bsp_normal_eq_jt_vec_", values, r, self.m, self.n, out)

    def jVec(self, values, v, out=None):
        """v [n] or [n, q] (leading B when values are batched) -> J v, [m] / [m, q] (bsp_normal_eq_j_vec_*)"""
        return self._run("jVec", "bsp_normal_eq_j_vec_", values, v, self.n, self.m, out)


class JacobianProduct(_EntryMap):
    """extension: products with the m x n Jacobian J of the entries (rows[k], cols[k],
    values[k]) (n = the solver's order(), caller's scalar order, no position repeated) taken from the entries
    alone: the lists of the rows and of the columns, each with its long runs, and the plan of the diagonal
    blocks of J^T J over the solver's params.  No layout, no pair list.  Built by Solver.jacobianProduct();
    keeps its solver alive.  jVec / jtVec are bitwise NormalEquations' (a run of more than 64 terms is summed
    by a whole wave in the same sequential order); the pieces of the matrix-free least squares built on them
    are driven by baspacho_amd.cgls."""

    _C = "jac_product"
    _KEYS = ("nnz", "m", "n", "max_row", "long_rows", "max_col", "long_cols", "row_bytes", "col_bytes")

    def __init__(self, solver, rows, cols, m):
        self._create("jacobianProduct", solver, rows, cols, before=(ctypes.c_int64(int(m)),))
        self.m = int(m)
        self.n = solver.order()

    _run = NormalEquations._run  # (values, a vector of one side, the output of the other: the same checks)

    def runTable(self, which):
        """(start, entry, index, long_runs) of the "rows" or the "cols" list: int32 arrays; the terms of run u
        are (entry[t], index[t]), t in [start[u], start[u + 1]), in ascending entry index; long_runs lists the
        runs of more than 64 terms"""
        if which not in ("rows", "cols"):
            raise ValueError("runTable: which must be 'rows' or 'cols', got %r" % (which,))
        runs = self.m if which == "rows" else self.n
        start = np.zeros(runs + 1, dtype=np.int32)
        entry, index = np.zeros(max(self.nnz, 1), dtype=np.int32), np.zeros(max(self.nnz, 1), dtype=np.int32)
        longs = np.zeros(max(runs, 1), dtype=np.int32)
        _check(self._lib.bsp_jac_product_table(self._h, ctypes.c_int32(0 if which == "rows" else 1),
                                               *(a.ctypes.data_as(_I32P) for a in (start, entry, index, longs)), None))
        return start, entry[:self.nnz], index[:self.nnz], longs[:int((np.diff(start) > 64).sum())]

    def precondInfo(self, kind):
        """{blocks, items, inverse_elems, max_width, device_bytes} of the plan of "jacobi" or "block_jacobi" for
        J^T J + D (the solver's params; one wider than 32 scalars is refused).  Host work only."""
        kinds = {"jacobi": 1, "block_jacobi": 2}
        if kind not in kinds:
            raise ValueError("precondInfo: kind must be 'jacobi' or 'block_jacobi', got %r" % (kind,))
        out = (ctypes.c_int64 * 5)()
        _check(self._lib.bsp_cgls_precond_info(self._h, ctypes.c_int32(kinds[kind]), out))
        return dict(zip(("blocks", "items", "inverse_elems", "max_width", "device_bytes"), [int(x) for x in out]))

    def blockTable(self):
        """(block_start, item_start, ka, kb, pos) of the plan of the diagonal blocks of J^T J: int32 arrays; the
        items of block b are t in [item_start[b], item_start[b + 1]), in ascending Jacobian row"""
        info = self.precondInfo("block_jacobi")
        nb, items = info["blocks"], info["items"]
        bs, st = np.zeros(nb + 1, dtype=np.int32), np.zeros(nb + 1, dtype=np.int32)
        ka, kb, pos = (np.zeros(max(items, 1), dtype=np.int32) for _ in range(3))
        _check(self._lib.bsp_jac_product_table(self._h, ctypes.c_int32(2),
                                               *(a.ctypes.data_as(_I32P) for a in (bs, st, ka, kb, pos))))
        return bs, st, ka[:items], kb[:items], pos[:items]

    def jtVec(self, values, r, out=None):
        """r [m] or [m, q] (leading B when values are batched) -> J^T r, [n] / [n, q] (bsp_jac_product_jtv_*)"""
        return self._run("jtVec", "bsp_jac_product_jtv_", values, r, self.m, self.n, out)

    def jVec(self, values, v, out=None):
        """v [n] or [n, q] (leading B when values are batched) -> J v, [m] / [m, q] (bsp_jac_product_jv_*)"""
        return self._run("jVec", "bsp_jac_product_jv_", values, v, self.n, self.m, out)


class JacobianSchur:
    """extension: implicit Schur elimination on the entries of a Jacobian.  The params
    `eliminate` of the JacobianProduct's solver are eliminated exactly (no Jacobian row may touch two of them, each
    has at most 8 scalars) and the reduced system S x_k = b_k, S = C - F^T B^-1 F, is reached through products
    alone: S and F are never formed.  Built by Solver.jacobianSchur(); keeps its product alive.  The kept scalars
    are numbered 0 .. nK - 1 and the eliminated ones 0 .. nE - 1 in ascending caller's scalar.  build: the inverses
    of the diagonal blocks of B = J_e^T J_e + D_e; mv: S p; reduce: b_k = g_k - F^T B^-1 g_e; backSubstitute: the
    full x from x_k.  Sums run in a fixed order with every product rounded first (bitwise the numpy restatement);
    each part of the map is uploaded by the first call that needs it; everything runs on the solver's stream
    without synchronising."""

    _KEYS = ("nnz", "m", "n", "n_kept", "n_elim", "elim_params", "free_rows", "max_elim_width", "max_group",
             "kept_entries", "elim_entries", "long_rows_kept", "long_rows_elim", "long_cols_elim", "long_cols_kept",
             "block_items", "inverse_elems", "map_bytes", "plan_bytes", "group_rows")

    def __init__(self, product, eliminate):
        self._lib = product._lib
        self._h = None
        e = _host_indices(eliminate, "eliminate")
        h = ctypes.c_void_p()
        _check(self._lib.bsp_jac_schur_create(product._h, ctypes.c_int64(len(e)), e.ctypes.data_as(_I64P),
                                              ctypes.byref(h)))
        self._h = h
        self.product, self.solver = product, product.solver
        self.m, self.n, self.nnz = product.m, product.n, product.nnz
        i = self.info()
        self.nK, self.nE, self.inverse_elems = i["n_kept"], i["n_elim"], i["inverse_elems"]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.bsp_jac_schur_destroy(h)

    def info(self):
        """figures of the map (bsp_jac_schur_info)"""
        out = (ctypes.c_int64 * len(self._KEYS))()
        _check(self._lib.bsp_jac_schur_info(self._h, out))
        return dict(zip(self._KEYS, [int(x) for x in out]))

    def table(self):
        """every list of the map as int32 arrays (bsp_jac_schur_table): a dict with rows_kept, rows_elim, cols_elim
        and cols_kept, each (start, entry, index, long_runs); kept_scalar, elim_scalar, elim_off, elim_param;
        group_start, group_row, free_rows; block_start, block_width, item_start, item_a, item_b, item_pos"""
        i = self.info()

        def get(part, *sizes):
            arrs = [np.zeros(max(n, 1), dtype=np.int32) for n in sizes]
            ptrs = [a.ctypes.data_as(_I32P) for a in arrs] + [None] * (4 - len(arrs))
            _check(self._lib.bsp_jac_schur_table(self._h, ctypes.c_int32(part), *ptrs))
            return [a[:n] for a, n in zip(arrs, sizes)]

        out = {}
        lists = (("rows_kept", self.m, i["kept_entries"], i["long_rows_kept"]),
                 ("rows_elim", self.m, i["elim_entries"], i["long_rows_elim"]),
                 ("cols_elim", self.nE, i["elim_entries"], i["long_cols_elim"]),
                 ("cols_kept", self.nK, i["kept_entries"], i["long_cols_kept"]))
        for part, (name, runs, items, longs) in enumerate(lists):
            out[name] = tuple(get(part, runs + 1, items, items, longs))
        ne = i["elim_params"]
        out["kept_scalar"], out["elim_scalar"], out["elim_off"], out["elim_param"] = get(4, self.nK, self.nE, ne + 1, ne)
        out["group_start"], out["group_row"], out["free_rows"] = get(5, ne + 1, i["group_rows"], i["free_rows"])
        out["block_start"], out["block_width"], out["item_start"] = get(6, ne + 1, ne, ne + 1)
        out["item_a"], out["item_b"], out["item_pos"] = get(7, *([i["block_items"]] * 3))
        return out

    _KINDS = {"jacobi": 1, "block_jacobi": 2}

    def precondInfo(self, kind):
        """{blocks, items, inverse_elems, max_width, device_bytes} of the plan of "jacobi" or "block_jacobi" for the
        reduced system, on the kept scalars (a kept param wider than 32 scalars is refused by name).  Host work only."""
        if kind not in self._KINDS:
            raise ValueError("precondInfo: kind must be 'jacobi' or 'block_jacobi', got %r" % (kind,))
        out = (ctypes.c_int64 * 5)()
        _check(self._lib.bsp_jac_schur_precond_info(self._h, ctypes.c_int32(self._KINDS[kind]), out))
        return dict(zip(("blocks", "items", "inverse_elems", "max_width", "device_bytes"), [int(x) for x in out]))

    def keptBlockTable(self):
        """(block_start, block_width, item_start, param, ka, kb, pos) of the plan of the diagonal blocks of C over the
        kept params: int32 arrays, block_start in the caller's scalars"""
        info = self.precondInfo("block_jacobi")
        nb, items = info["blocks"], info["items"]
        a = [np.zeros(max(n, 1), dtype=np.int32) for n in (nb + 1, nb, nb + 1, nb)]
        _check(self._lib.bsp_jac_schur_table(self._h, ctypes.c_int32(8), *(x.ctypes.data_as(_I32P) for x in a)))
        b = [np.zeros(max(items, 1), dtype=np.int32) for _ in range(3)]
        _check(self._lib.bsp_jac_schur_table(self._h, ctypes.c_int32(9), *(x.ctypes.data_as(_I32P) for x in b), None))
        return a[0], a[1][:nb], a[2], a[3][:nb], b[0][:items], b[1][:items], b[2][:items]

    def precondBuild(self, kind, values, colsq=None, d=None):
        """(minv, status) of the built-in preconditioner `kind` of the reduced system for the entry values [nnz] /
        [B, nnz] (bsp_jac_schur_precond_build_*): "jacobi" from the column norms colsq [n] / [B, n] (float64),
        "block_jacobi" from the values; d: the damping vector or None.  status as build()'s."""
        import torch
        if kind not in self._KINDS:
            raise ValueError("precondBuild: kind must be 'jacobi' or 'block_jacobi', got %r" % (kind,))
        lead = self._lead("precondBuild", values)
        batched = len(lead) == 1
        if kind == "jacobi" and (not isinstance(colsq, torch.Tensor) or colsq.dtype != torch.float64
                                 or tuple(colsq.shape) != lead + (self.n,) or colsq.device != values.device):
            raise ValueError("precondBuild: colsq must be the float64 column norms %s" % (lead + (self.n,),))
        if d is not None and self._operand("precondBuild", "d", d, values, lead, self.n) is not None:
            raise ValueError("precondBuild: d must be [n] or [B, n]")
        elems = self.precondInfo(kind)["inverse_elems"]
        minv = torch.empty(lead + (max(elems, 1),), dtype=values.dtype, device=values.device)
        status = torch.empty(lead + (2,), dtype=torch.int64, device=values.device)
        need = ctypes.c_int64(0)
        _check(self._lib.bsp_cgls_work_bytes(self.solver._h, self.product._h, ctypes.c_int64(1), ctypes.byref(need)))
        nb = values.shape[0] if batched else 1
        work = torch.empty(need.value * nb + 16, dtype=torch.uint8, device=values.device)
        mem = self._members
        if colsq is not None:
            _ptr_of(colsq)
        _call(self._lib, "bsp_jac_schur_precond_build_", batched, _suffix(values), self.solver._h, self._h,
              ctypes.c_int32(self._KINDS[kind]), mem(values, batched), mem(colsq if kind == "jacobi" else None, batched),
              mem(d, batched), mem(minv, batched), ctypes.c_void_p((work.data_ptr() + 15) // 16 * 16),
              ctypes.c_void_p(_ptr_of(status)), *((ctypes.c_int32(nb),) if batched else ()))
        return minv, status

    # ---- the block diagonal of S as preconditioner
    _SJ_KEYS = ("blocks", "real_pairs", "pseudo_pairs", "pair_rows", "chunks", "inverse_elems", "partial_elems",
                "device_bytes")

    def schurJacobiInfo(self):
        """figures of the plan of "schur_jacobi", the block diagonal of S over the kept params (bsp_jac_schur_sjacobi_info;
        a kept param wider than 32 scalars is refused by name), and kept_item_plan_built: whether the item plan of
        "block_jacobi" exists, which this plan never needs.  Host work only; the plan is built by the first call."""
        out = (ctypes.c_int64 * 8)()
        _check(self._lib.bsp_jac_schur_sjacobi_info(self._h, out))
        info = dict(zip(self._SJ_KEYS, [int(x) for x in out]))
        built = ctypes.c_int32(0)
        _check(self._lib.bsp_jac_schur_kept_plan_built(self._h, ctypes.byref(built)))
        info["kept_item_plan_built"] = bool(built.value)
        return info

    def schurJacobiTable(self):
        """every table of that plan (bsp_jac_schur_sjacobi_table): block_pair, block_chunk, block_width, block_off
        (int64); chunk_pair, chunk_block, chunk_part (int64); pair_elim, pair_row, pair_rec; row_of, rec"""
        i = self.schurJacobiInfo()
        nb, nc, npairs = i["blocks"], i["chunks"], i["real_pairs"] + i["pseudo_pairs"]

        def get(part, sizes, size64=None):
            arrs = [np.zeros(max(n, 1), dtype=np.int32) for n in sizes]
            ptrs = [a.ctypes.data_as(_I32P) for a in arrs] + [None] * (3 - len(arrs))
            wide = None if size64 is None else np.zeros(max(size64, 1), dtype=np.int64)
            _check(self._lib.bsp_jac_schur_sjacobi_table(self._h, ctypes.c_int32(part), *ptrs,
                                                         None if wide is None else wide.ctypes.data_as(_I64P)))
            return [a[:n] for a, n in zip(arrs, sizes)] + ([] if wide is None else [wide[:size64]])

        out = {}
        out["block_pair"], out["block_chunk"], out["block_width"], out["block_off"] = get(0, (nb + 1, nb + 1, nb), nb + 1)
        out["chunk_pair"], out["chunk_block"], out["chunk_part"] = get(1, (nc + 1, nc), nc + 1)
        out["pair_elim"], out["pair_row"], out["pair_rec"] = get(2, (npairs, npairs + 1, npairs + 1))
        out["row_of"], out["rec"] = get(3, (i["pair_rows"], int(out["pair_rec"][-1])))
        return out

    def schurJacobiBuild(self, values, binv, d=None, partials=None, out=None):
        """(minv, status): the inverses of the diagonal blocks of S = C - F^T B^-1 F over the kept params, [inverse_elems]
        / [B, inverse_elems], block b row-major at the offsets of "block_jacobi"'s kept blocks, and status as build()'s
        (bsp_jac_schur_sjacobi_build_*).  binv: what build() returned for these values and d; d: the damping vector or
        None; partials: float64 scratch [partial_elems] / [B, partial_elems] for the chunk sums (allocated when
        None); out: where minv goes.  All block arithmetic is in float64; a bad block gets a zero inverse."""
        import torch
        name = "schurJacobiBuild"
        lead = self._lead(name, values)
        batched = len(lead) == 1
        if (not isinstance(binv, torch.Tensor) or binv.dtype != values.dtype or binv.device != values.device
                or tuple(binv.shape) != lead + (max(self.inverse_elems, 1),)):
            raise ValueError("%s: binv must be what build() returned for these values" % name)
        _ptr_of(binv)
        if d is not None and self._operand(name, "d", d, values, lead, self.n) is not None:
            raise ValueError("%s: d must be [n] or [B, n]" % name)
        info = self.schurJacobiInfo()
        pshape = lead + (max(info["partial_elems"], 1),)
        if partials is None:
            partials = torch.empty(pshape, dtype=torch.float64, device=values.device)
        elif (not isinstance(partials, torch.Tensor) or partials.dtype != torch.float64 or partials.device != values.device
              or tuple(partials.shape) != pshape):
            raise ValueError("%s: partials must be a float64 tensor of shape %s on %s" % (name, pshape, values.device))
        minv = _EntryMap._alloc_out(name, values, lead + (max(info["inverse_elems"], 1),), out)
        _ptr_of(partials), _ptr_of(minv)
        status = torch.empty(lead + (2,), dtype=torch.int64, device=values.device)
        need = ctypes.c_int64(0)
        _check(self._lib.bsp_cgls_work_bytes(self.solver._h, self.product._h, ctypes.c_int64(1), ctypes.byref(need)))
        nb = values.shape[0] if batched else 1
        work = torch.empty(need.value * nb + 16, dtype=torch.uint8, device=values.device)
        mem = self._members
        _call(self._lib, "bsp_jac_schur_sjacobi_build_", batched, _suffix(values), self.solver._h, self._h,
              mem(values, batched), mem(binv, batched), mem(d, batched), mem(partials, batched), mem(minv, batched),
              ctypes.c_void_p((work.data_ptr() + 15) // 16 * 16), ctypes.c_void_p(_ptr_of(status)),
              *((ctypes.c_int32(nb),) if batched else ()))
        return minv, status

    def schurJacobiApply(self, minv, r, z, work, state):
        """the preconditioner piece of a conjugate gradient on the kept scalars with the minv of schurJacobiBuild
        (bsp_jac_schur_sjacobi_apply_*): z = M^-1 r, r.z and beta for the running columns of `state`.  r, z: [nK, q]
        ([B, nK, q] with minv [B, inverse_elems]); work: the iteration's 16-byte aligned device work area as a
        ctypes pointer or an int address; state: its int64 records [.., q, 12].  Never builds the item plan of
        "block_jacobi"."""
        import torch
        name = "schurJacobiApply"
        if not isinstance(minv, torch.Tensor) or minv.dim() not in (1, 2):
            raise ValueError("%s: minv must be what schurJacobiBuild() returned" % name)
        batched = minv.dim() == 2
        lead = tuple(minv.shape[:-1])
        for what, t in (("r", r), ("z", z)):
            if (not isinstance(t, torch.Tensor) or t.dtype != minv.dtype or t.device != minv.device
                    or t.dim() != len(lead) + 2 or tuple(t.shape[:-1]) != lead + (self.nK,) or t.shape[-1] < 1
                    or t.shape != r.shape):
                raise ValueError("%s: %s must be a %s tensor %s on %s" % (name, what, minv.dtype, lead + (self.nK, "q"),
                                                                         minv.device))
            _ptr_of(t)
        q = int(r.shape[-1])
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.int64 or tuple(state.shape) != lead + (q, 12)
                or state.device != minv.device):
            raise ValueError("%s: state must be the int64 records %s of a CgRun" % (name, lead + (q, 12)))
        _ptr_of(minv)
        mem = self._members
        work = work if isinstance(work, ctypes.c_void_p) else ctypes.c_void_p(int(work))
        _call(self._lib, "bsp_jac_schur_sjacobi_apply_", batched, _suffix(minv), self.solver._h, self._h, ctypes.c_int64(q),
              mem(minv, batched), mem(r, batched), mem(z, batched), work, ctypes.c_void_p(_ptr_of(state)),
              *((ctypes.c_int32(minv.shape[0]),) if batched else ()))
        return z

    # ---- the device entries: values [nnz] / [B, nnz]; vectors [rows] / [rows, q] with a leading B for a batch
    def _lead(self, name, values):
        import torch
        if not isinstance(values, torch.Tensor):
            raise TypeError("%s: values must be a torch.Tensor, got %s" % (name, type(values).__name__))
        if values.dim() not in (1, 2) or values.shape[-1] != self.nnz:
            raise ValueError("%s: values must be [%d] or [B, %d], got shape %s"
                             % (name, self.nnz, self.nnz, tuple(values.shape)))
        if values.dim() == 2 and values.shape[0] == 0:
            raise ValueError("%s: empty batch" % name)
        _ptr_of(values)
        return tuple(values.shape[:-1])

    def _operand(self, name, what, t, values, lead, rows, optional=False):
        """checks one operand against `values`; returns q (None: the operand is absent or has no vector axis)"""
        import torch
        if t is None:
            if optional:
                return None
            raise ValueError("%s: %s is missing" % (name, what))
        if not isinstance(t, torch.Tensor) or t.dtype != values.dtype or t.device != values.device:
            raise TypeError("%s: %s must be a %s tensor on %s" % (name, what, values.dtype, values.device))
        nl = len(lead)
        if t.dim() not in (nl + 1, nl + 2) or tuple(t.shape[:nl]) != lead or t.shape[nl] != rows:
            raise ValueError("%s: %s must be %s[%d] or [%d, q], got shape %s"
                             % (name, what, "[B, ...] " if nl else "", rows, rows, tuple(t.shape)))
        _ptr_of(t)
        if t.dim() == nl + 2 and t.shape[-1] < 1:
            raise ValueError("%s: %s has no vectors" % (name, what))
        return int(t.shape[-1]) if t.dim() == nl + 2 else None

    @staticmethod
    def _members(t, batched):
        return None if t is None else _ptr_arg(t.unbind(0) if batched else [t], batched)

    def build(self, values, d=None):
        """(binv, status): the inverses of the diagonal blocks of B = J_e^T J_e + D_e, [inverse_elems] /
        [B, inverse_elems], block e row-major, and status int64 [2] / [B, 2] = {the caller's scalar of the lowest
        bad pivot or -1, bad blocks} (bsp_jac_schur_build_*).  d: the damping vector [n] / [B, n] or None.  The
        blocks are bitwise those of cgls.Preconditioner(product, "block_jacobi", ...); a bad block gets a zero
        inverse."""
        import torch
        lead = self._lead("build", values)
        batched = len(lead) == 1
        if d is not None and (self._operand("build", "d", d, values, lead, self.n) is not None):
            raise ValueError("build: d must be [n] or [B, n]")
        binv = torch.empty(lead + (max(self.inverse_elems, 1),), dtype=values.dtype, device=values.device)
        status = torch.empty(lead + (2,), dtype=torch.int64, device=values.device)
        need = ctypes.c_int64(0)
        _check(self._lib.bsp_cgls_work_bytes(self.solver._h, self.product._h, ctypes.c_int64(1), ctypes.byref(need)))
        nb = values.shape[0] if batched else 1
        work = torch.empty(need.value * nb + 16, dtype=torch.uint8, device=values.device)
        mem = self._members
        _call(self._lib, "bsp_jac_schur_build_", batched, _suffix(values), self.solver._h, self._h, mem(values, batched),
              mem(d, batched), mem(binv, batched), ctypes.c_void_p((work.data_ptr() + 15) // 16 * 16),
              ctypes.c_void_p(_ptr_of(status)), *((ctypes.c_int32(nb),) if batched else ()))
        return binv, status

    def _run(self, name, values, binv, rows_out, ins, d=None, state=None, out=None, t=None):
        """ins: ((what, tensor, rows), ...) in the entry's order, all of one q"""
        import torch
        lead = self._lead(name, values)
        batched = len(lead) == 1
        if (not isinstance(binv, torch.Tensor) or binv.dtype != values.dtype or binv.device != values.device
                or tuple(binv.shape) != lead + (max(self.inverse_elems, 1),)):
            raise ValueError("%s: binv must be what build() returned for these values" % name)
        _ptr_of(binv)
        if d is not None and self._operand(name, "d", d, values, lead, self.n) is not None:
            raise ValueError("%s: d must be [n] or [B, n]" % name)
        qs = [self._operand(name, what, x, values, lead, rows) for what, x, rows in ins]
        if any(qi != qs[0] for qi in qs):
            raise ValueError("%s: the vectors must have one shape [rows] or [rows, q]" % name)
        q = 1 if qs[0] is None else qs[0]
        tail = () if qs[0] is None else (q,)
        out = _EntryMap._alloc_out(name, values, lead + (rows_out,) + tail, out)
        t = _EntryMap._alloc_out(name + " scratch", values, lead + (self.m, q), t)
        _ptr_of(out), _ptr_of(t)
        mem = self._members
        args = [mem(values, batched), mem(binv, batched)]
        if name == "mv":
            args.append(mem(d, batched))
        args += [mem(x, batched) for _, x, _ in ins] + [mem(t, batched), mem(out, batched)]
        if name == "mv":
            if state is not None:
                if state.dtype != torch.int64 or tuple(state.shape) != lead + (q, 12):
                    raise ValueError("mv: state must be the int64 records %s of a CgRun" % (lead + (q, 12),))
                args.append(ctypes.c_void_p(_ptr_of(state)))
            else:
                args.append(None)
        _call(self._lib, "bsp_jac_schur_%s_" % {"backSubstitute": "back"}.get(name, name), batched, _suffix(values),
              self.solver._h, self._h, ctypes.c_int64(q), *args, *((ctypes.c_int32(values.shape[0]),) if batched else ()))
        return out

    def mv(self, values, binv, p, d=None, state=None, out=None, t=None):
        """p [nK] or [nK, q] (leading B when values are batched) -> S p (bsp_jac_schur_mv_*).  d: the damping vector
        or None; state: the records of a cg.CgRun, whose stopped columns are then left untouched; t: scratch
        [.., m, q]"""
        return self._run("mv", values, binv, self.nK, (("p", p, self.nK),), d=d, state=state, out=out, t=t)

    def reduce(self, values, binv, g, out=None, t=None):
        """g [n] or [n, q], the full right-hand side J^T r + c -> b_k = g_k - F^T B^-1 g_e, [nK] / [nK, q]
        (bsp_jac_schur_reduce_*)"""
        return self._run("reduce", values, binv, self.nK, (("g", g, self.n),), out=out, t=t)

    def backSubstitute(self, values, binv, g, xk, out=None, t=None):
        """x [n] / [n, q] in the caller's order from the reduced solution xk [nK] / [nK, q]: the kept scalars are
        xk's, the eliminated ones B^-1 (g_e - F x_k) (bsp_jac_schur_back_*)"""
        return self._run("backSubstitute", values, binv, self.n, (("g", g, self.n), ("xk", xk, self.nK)), out=out, t=t)


class SymProduct(_EntryMap):
    """extension: products with the symmetric matrix A of the coordinate entries
    (rows[k], cols[k], values[k]) in the caller's scalar order, taken straight from the entries: the solver's
    layout is never built.  Built by Solver.symProduct(); keeps its solver alive.  A is the matrix
    Solver.assembly() builds from the same entries (same triangle and index rules).  mv: A x; outer: the
    gradient of the values of sum(g * (A x)).  Sums run in a fixed order with every product rounded first
    (bitwise the numpy restatement); each part of the map is uploaded by the first call that needs it;
    everything runs on the solver's stream without synchronising."""

    _C = "sym_product"
    _KEYS = ("nnz", "kept", "terms", "max_row", "long_rows", "device_bytes")

    def __init__(self, solver, rows, cols, triangle="lower"):
        if triangle not in _TRIANGLES:
            raise ValueError("symProduct: triangle must be 'lower' or 'full', got %r" % (triangle,))
        self._create("symProduct", solver, rows, cols, after=(ctypes.c_int32(_TRIANGLES[triangle]),))
        self.n = solver.order()
        self.triangle = triangle

    def rowTable(self):
        """(row_start, entry, index): the terms of row i are (entry[t], index[t]), t in [row_start[i],
        row_start[i + 1]); int32 arrays of order() + 1, info()["terms"] and info()["terms"] values"""
        T = self.info()["terms"]
        start = np.empty(self.n + 1, dtype=np.int32)
        entry, index = np.empty(T, dtype=np.int32), np.empty(T, dtype=np.int32)
        _check(self._lib.bsp_sym_product_row_table(self._h, start.ctypes.data_as(_I32P),
                                                   entry.ctypes.data_as(_I32P), index.ctypes.data_as(_I32P)))
        return start, entry, index

    def cgPrecondTable(self, kind):
        """the host plan of a built-in preconditioner of the conjugate gradient, kind
        "jacobi" or "block_jacobi" (the solver's params; one wider than 32 scalars is refused): (block_start,
        item_start, entry, pos, info).  The items of block b are (entry[t], pos[t]), t in [item_start[b],
        item_start[b + 1]), in ascending entry index: the kept entries (i, j), i >= j, inside the block, pos =
        (i - s) w + (j - s); info = {blocks, items, inverse_elems, max_width}.  Host work only."""
        kinds = {"jacobi": 1, "block_jacobi": 2}
        if kind not in kinds:
            raise ValueError("cgPrecondTable: kind must be 'jacobi' or 'block_jacobi', got %r" % (kind,))
        k = ctypes.c_int32(kinds[kind])
        out = (ctypes.c_int64 * 4)()
        _check(self._lib.bsp_cg_precond_info(self._h, k, out))
        nb, items = int(out[0]), int(out[1])
        bs, st = np.empty(nb + 1, dtype=np.int32), np.empty(nb + 1, dtype=np.int32)
        entry, pos = np.empty(items, dtype=np.int32), np.empty(items, dtype=np.int32)
        _check(self._lib.bsp_cg_precond_table(self._h, k, bs.ctypes.data_as(_I32P), st.ctypes.data_as(_I32P),
                                              entry.ctypes.data_as(_I32P), pos.ctypes.data_as(_I32P)))
        return bs, st, entry, pos, {"blocks": nb, "items": items, "inverse_elems": int(out[2]), "max_width": int(out[3])}

    def cgFsaiTable(self):
        """the host plan of the "fsai" preconditioner of the conjugate gradient: a dict of
        int32 arrays and info.  Row i of G sits on the scalars cols[row_start[i] : row_start[i + 1]], ascending,
        i last (the 31 largest of the earlier ones when there are more); its items are (entry[t], pos[t]), t in
        [item_start[i], item_start[i + 1]), in ascending entry index, pos = la w + lb in the row's local matrix;
        column j of G is (col_pos[t], col_row[t]), t in [col_start[j], col_start[j + 1]), rows ascending; long_cols
        lists the columns of more than 64 terms; info = {rows, items, elems, max_width}.  Host work only."""
        out = (ctypes.c_int64 * 4)()
        _check(self._lib.bsp_cg_precond_info(self._h, ctypes.c_int32(3), out))
        n, items, elems = int(out[0]), int(out[1]), int(out[2])
        sizes = {"row_start": n + 1, "cols": elems, "item_start": n + 1, "entry": items, "pos": items,
                 "col_start": n + 1, "col_pos": elems, "col_row": elems, "long_cols": n}
        t = {k: np.zeros(max(v, 1), dtype=np.int32) for k, v in sizes.items()}
        _check(self._lib.bsp_fsai_table(self._h, *(a.ctypes.data_as(_I32P) for a in t.values())))
        t = {k: a[:sizes[k]] for k, a in t.items()}
        t["long_cols"] = t["long_cols"][:int((np.diff(t["col_start"]) > 64).sum())]
        t["info"] = {"rows": n, "items": items, "elems": elems, "max_width": int(out[3])}
        return t

    def _run(self, name, fn, a, a_what, x, out, batched):
        """a: values [nnz] / [B, nnz] (mv) or g, shaped like x (outer); x [n] / [n, q], or those with a
        leading B when `batched`; out [.., n(, q)] (mv) or [.., nnz] (outer)"""
        sfx, shape, q = self._operands(name, a, a_what, x, batched)
        return self._launch(name, fn, sfx, [a, x], shape, out, batched, q)

    def _operands(self, name, a, a_what, x, batched):
        """the checks of _run's operands: (suffix of the entry, shape of the output, q)"""
        import torch
        for what, t in ((a_what, a), ("x", x)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a torch.Tensor, got %s" % (name, what, type(t).__name__))
        if x.dtype != a.dtype or x.device != a.device:
            raise TypeError("%s: x is %s on %s, %s is %s on %s" % (name, x.dtype, x.device, a_what, a.dtype, a.device))
        sfx = _suffix(a)
        mv = a_what == "values"
        if mv and (a.dim() != (2 if batched else 1) or a.shape[-1] != self.nnz):
            raise ValueError("%s: values must be [%d] or [B, %d], got shape %s"
                             % (name, self.nnz, self.nnz, tuple(a.shape)))
        if not mv and a.shape != x.shape:
            raise ValueError("%s: g has shape %s, x has %s" % (name, tuple(a.shape), tuple(x.shape)))
        lo = 1 if batched else 0
        if x.dim() not in (lo + 1, lo + 2) or x.shape[lo] != self.n or (mv and x.shape[:lo] != a.shape[:lo]):
            raise ValueError("%s: x must be %s with n = %d, got shape %s" % (
                name, "[B, n] or [B, n, q]" if batched else "[n] or [n, q]", self.n, tuple(x.shape)))
        if batched and x.shape[0] == 0:
            raise ValueError("%s: empty batch" % name)
        has_q = x.dim() == lo + 2
        q = x.shape[-1] if has_q else 1
        if q < 1:
            raise ValueError("%s: x has no vectors" % name)
        shape = tuple(x.shape) if mv else tuple(x.shape[:lo]) + (self.nnz,)
        return sfx, shape, q

    def mv(self, values, x, out=None):
        """values [nnz] or [B, nnz] (device, float64 / float32); x [n] or [n, q] in the caller's order (leading
        B when values are batched) -> A x, shaped like x: every element written, +0 for a row without terms
        (bsp_sym_product_mv_*)"""
        import torch
        return self._run("mv", "bsp_sym_product_mv_", values, "values", x, out,
                         isinstance(values, torch.Tensor) and values.dim() == 2)

    def outer(self, g, x, out=None, batched=None):
        """g and x of one shape, [n] or [n, q], or those with a leading B -> the gradient of the values of
        sum(g * (A x)), [nnz] / [B, nnz]: sum_j g[r, j] x[c, j] (+ g[c, j] x[r, j] off the diagonal) at entry
        k = (r, c), 0 for skipped entries, the full value for every duplicate (bsp_sym_product_outer_*).
        Three dimensions are a batch, one is not; two are [n, q] unless batched=True or `out` is [B, nnz]"""
        import torch
        if batched is None:
            dims = x.dim() if isinstance(x, torch.Tensor) else 0
            batched = dims == 3 or (dims == 2 and isinstance(out, torch.Tensor) and out.dim() == 2)
        return self._run("outer", "bsp_sym_product_outer_", g, "g", x, out, bool(batched))

    # ---- error bounds; not differentiable ------------------------------------
    def absMv(self, values, x, out=None):
        """|A| |x|, shaped like x: row i is the terms |values[k]| * |x[idx]| of mv's list folded in the same
        order from +0, duplicates as separate terms, so that cancelling duplicates do not shrink it
        (bsp_sym_product_abs_mv_*).  Arguments as for mv; every element written.  Not differentiable."""
        import torch
        return self._run("absMv", "bsp_sym_product_abs_mv_", values, "values", x, out,
                         isinstance(values, torch.Tensor) and values.dim() == 2)

    def residual(self, values, x, b, out=None):
        """(r, d) of x as a solution of A x = b, both shaped like x, from ONE pass over mv's row lists
        (bsp_sym_product_residual_*): r = b - A x, bitwise b - mv(values, x), and d = |A| |x| + |b|, the
        Oettli-Prager denominator (absMv's terms, then |b| added).  values, x as for mv, b shaped like x;
        out: a pair (r, d) of tensors to write.  Every element of both is written.  Not differentiable."""
        import torch
        name = "residual"
        if not isinstance(b, torch.Tensor):
            raise TypeError("%s: b must be a torch.Tensor, got %s" % (name, type(b).__name__))
        batched = isinstance(values, torch.Tensor) and values.dim() == 2
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError("%s: out must be a pair (r, d) of tensors" % name)
        if isinstance(x, torch.Tensor) and (b.shape != x.shape or b.dtype != x.dtype or b.device != x.device):
            raise ValueError("%s: b must be %s %s on %s like x, got %s %s on %s" % (
                name, tuple(x.shape), x.dtype, x.device, tuple(b.shape), b.dtype, b.device))
        sfx, shape, q = self._operands(name, values, "values", x, batched)
        r, d = (None, None) if out is None else out
        r, d = self._alloc_out(name, x, shape, r), self._alloc_out(name, x, shape, d)
        ts = (values, x, b, r, d)
        for t in ts:
            _ptr_of(t)  # device memory, contiguous
        ptrs = [_ptr_arg(t.unbind(0) if batched else [t], batched) for t in ts]
        _call(self._lib, "bsp_sym_product_residual_", batched, sfx, self.solver._h, self._h, *ptrs[:3],
              ctypes.c_int64(q), ptrs[3], ptrs[4], *_count(d, batched))
        return r, d


def probe_mfma_f64_tflops():
    """sustained fp64 MFMA rate of the current GPU (register-only probe kernel), TFLOP/s"""
    out = ctypes.c_double(0)
    _check(_lib.load().bsp_probe_mfma_f64(ctypes.byref(out)))
    return out.value


def debug_read_trace(max_records=8192):
    """in-situ kernel clock records (library built with BSP_KTRACE=1), array [n, 8]"""
    out = np.zeros((max_records, 8), dtype=np.int64)
    n = ctypes.c_int(0)
    _check(_lib.load().bsp_debug_read_trace(out.ctypes.data_as(ctypes.c_void_p), max_records,
                                            ctypes.byref(n)))
    return out[:n.value]


def debug_read_extents(max_launches=2048):
    """per chain-step launch [first start, last start, last end, workgroup-0 end] (trace builds)"""
    out = np.zeros((max_launches, 4), dtype=np.uint64)
    n = ctypes.c_int(0)
    _check(_lib.load().bsp_debug_read_extents(out.ctypes.data_as(ctypes.c_void_p), max_launches,
                                              ctypes.byref(n)))
    return out[:n.value]


def create_solver(settings: Optional[Settings], param_sizes, ss: SparseStructure,
                  sparse_elim_ranges=(), elim_last_ids=()) -> Solver:
    """createSolver (Solver.h:235-237): symbolic analysis on the host; never touches the GPU."""
    lib = _lib.load()
    st = settings or Settings()
    cs = _CSettings(int(st.findSparseEliminationRanges), int(st.numThreads), int(st.backend),
                    int(st.addFillPolicy), None)
    model = None
    if st.computationModel is not None:
        model = (ctypes.c_double * 20)(*[float(x) for x in st.computationModel])
        cs.computation_model = ctypes.cast(model, ctypes.POINTER(ctypes.c_double))
    ps = _i64(param_sizes)
    if len(ps) != ss.order():
        raise ValueError("param_sizes and sparse structure disagree on the number of params")
    er, el = _i64(sparse_elim_ranges), _i64(sorted(elim_last_ids))
    h = ctypes.c_void_p()
    ho = None
    if st.hipOptions:
        ho = _CHipOptions()
        lib.bsp_hip_options_default(ctypes.byref(ho))
        for k, v in st.hipOptions.items():
            if k in _HIP_OPTION_INTS:
                setattr(ho, k, int(v))
            elif k in _HIP_OPTION_REALS:
                setattr(ho, k, float(v))
            else:
                raise ValueError("unknown backend option %r (bsp_hip_options has: %s)" %
                                 (k, ", ".join(_HIP_OPTION_INTS + _HIP_OPTION_REALS)))
    _check(lib.bsp_create_solver_opts(
        ctypes.byref(cs), ctypes.byref(ho) if ho is not None else None,
        ctypes.c_int64(len(ps)), ps.ctypes.data_as(_I64P),
        ss.ptrs.ctypes.data_as(_I64P), ss.inds.ctypes.data_as(_I64P), ctypes.c_int64(len(er)),
        er.ctypes.data_as(_I64P), ctypes.c_int64(len(el)), el.ctypes.data_as(_I64P),
        ctypes.byref(h)))
    return Solver(h)
