// What the translation units of the MI355X backend share (hip_backend.hip, hip_factor.hip,
// hip_solve.hip, hip_extensions.hip): device plumbing, the uploaded plan and the symbolic context.
// PRIVATE: included by those four files only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>

#include "backend_options.h"
#include "hip_backend.h"
#include "hip_device_common.h"
#include "hip_plan.h"
#include "mat_ops.h"

namespace BaSpaCho {

#define hipCHECK(expr)                                                                    \
  do {                                                                                    \
    hipError_t bsp_err_ = (expr);                                                         \
    if (bsp_err_ != hipSuccess) {                                                         \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(bsp_err_) + \
                               " in " #expr " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    }                                                                                     \
  } while (0)

// internal to the backend: these types cross its translation units, nothing outside them sees them
namespace hipb {

using std::vector;

// owning device array
struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  DevBuf() {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
  ~DevBuf() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
  void resize(size_t n) {
    if (n <= bytes) return;
    release();
    hipCHECK(hipMalloc(&ptr, n));
    bytes = n;
  }
  template <typename U>
  void upload(const vector<U>& v) {
    resize(std::max<size_t>(v.size() * sizeof(U), 16));
    if (!v.empty()) hipCHECK(hipMemcpy(ptr, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice));
  }
  template <typename U>
  const U* as() const { return reinterpret_cast<const U*>(ptr); }
};

// per level list of a plan and schedule mode (0: levels + block groups, 1: with sweeps): the steps,
// and the panels whose diagonal blocks are inverted (built and uploaded on the first solve)
struct SolveInvList : SolveSchedule {
  bool built = false;
  int64_t count = 0;
  DevBuf list;
};

struct DevPlan {
  HipPlanHost host;
  // keyed by the address of a level list that lives inside `host` (host.levels, an elimination
  // range's bigLevels): the entries die with the plan, an address is never reused under them
  std::map<std::pair<const void*, int>, SolveInvList> solveInvLists;
  DevBuf panels, levelPanelDescs, trsmTasksFat, chainOffTab, rowChain, rowLocal, rowColOff, levelPanels, trsmTasks,
      updTasksFat, updTasksWide, elimChainLump, elimItems, elimPairOffJ, elimPairOffI, rowGlobal, elimLumpDesc;
  int64_t numUpdTasks = 0;
  vector<int64_t> slowPrefix;  // tasks [0, i) that updateTileBulk cannot take
  // split-K task lists of small multi-panel levels: level's updBegin -> [begin, end) in updTasksSplit
  DevBuf updTasksSplit;
  std::map<int64_t, std::pair<int64_t, int64_t>> splitRange;
  // potrf folded into the trsm launch of small multi-panel levels (LaunchTables, hip_plan.h)
  DevBuf foldDescs;
  vector<int32_t> foldRank;      // per level of host.levels: position in the sorted order, -1: not foldable
  vector<int64_t> foldTiles;     // sorted order: row tiles of the level
  vector<int64_t> foldPanelEnd;  // ... panels of the levels up to and including this one
  // forward-solve gather lists, built on the first solve that needs them
  bool solveGatherReady = false;
  SolveGatherPlan solveGather;
  DevBuf solveEntries, solveItems, solveLumpBlocks, solveLumpDescs;
  void ensureSolveGather(const CoalescedBlockMatrixSkel& skel) {
    if (solveGatherReady) return;
    solveGather = buildSolveGather(skel, host);
    solveEntries.upload(solveGather.entries);
    solveItems.upload(solveGather.items);
    solveLumpBlocks.upload(solveGather.lumpBlocks);
    solveLumpDescs.upload(solveGather.lumpDescs);
    vector<SolveGatherEntry>().swap(solveGather.entries);
    vector<SolveLumpBlock>().swap(solveGather.lumpBlocks);
    vector<SolveLumpDesc>().swap(solveGather.lumpDescs);
    solveGatherReady = true;
  }
  void upload() {
    panels.upload(host.panels);
    chainOffTab.upload(host.chainOffTab);
    rowChain.upload(host.rowChain);
    rowLocal.upload(host.rowLocal);
    rowColOff.upload(host.rowColOff);
    rowGlobal.upload(host.rowGlobal);
    levelPanels.upload(host.levelPanels);
    trsmTasks.upload(host.trsmTasks);
    LaunchTables tab = buildLaunchTables(host);
    levelPanelDescs.upload(tab.levelPanelDescs);
    trsmTasksFat.upload(tab.trsmTasksFat);
    foldDescs.upload(tab.foldDescs);
    updTasksFat.upload(tab.updTasksFat);
    updTasksWide.upload(tab.updTasksWide);
    updTasksSplit.upload(tab.updTasksSplit);
    slowPrefix = std::move(tab.slowPrefix);
    splitRange = std::move(tab.splitRange);
    foldRank = std::move(tab.foldRank);
    foldTiles = std::move(tab.foldTiles);
    foldPanelEnd = std::move(tab.foldPanelEnd);
    elimChainLump.upload(host.elimChainLump);
    elimLumpDesc.upload(host.elimLumpDesc);
    elimItems.upload(host.elimItems);
    elimPairOffJ.upload(host.elimPairOffJ);
    elimPairOffI.upload(host.elimPairOffI);
    // the launch code only needs the descriptors it passes by value and the level / range
    // tables: release the host copies of everything that now lives on the device (BAL-871:
    // 0.3 GB of pair offsets and task lists)
    numUpdTasks = (int64_t)host.updTasks.size();
    auto drop = [](auto& v) { std::decay_t<decltype(v)>().swap(v); };
    drop(host.chainOffTab);
    drop(host.rowChain);
    drop(host.rowLocal);
    drop(host.rowColOff);
    drop(host.rowGlobal);
    drop(host.levelPanels);
    drop(host.trsmTasks);
    drop(host.updTasks);
    drop(host.elimChainLump);
    drop(host.elimLumpDesc);
    drop(host.elimItems);
    drop(host.elimPairOffJ);
    drop(host.elimPairOffI);
  }
};

// Pointer arrays of a batched call (one device pointer per matrix / vector) travel through a small
// ring of pinned host slots and device slots, copied on the execution stream: no synchronous
// hipMemcpy, no per-call allocation, and a slot is not rewritten while an earlier call's kernels
// may still read it (the reference re-uploads the array for every op, MatOpsCuda.cu:730,761,788).
struct PtrRing {
  static constexpr int kSlots = 32;
  char* host = nullptr;
  DevBuf dev;
  size_t slotBytes = 0;
  int next = 0;
  hipEvent_t ev[kSlots] = {};
  bool used[kSlots] = {};
  ~PtrRing() { release(); }
  void release() {
    for (int i = 0; i < kSlots; i++) {
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      ev[i] = nullptr;
      used[i] = false;
    }
    if (host) (void)hipHostFree(host);
    host = nullptr;
    dev.release();
    slotBytes = 0;
  }
  // slots of at least `bytes`.  Growing (the first call, or a larger array than ever before) waits for
  // the device and allocates all slots anew: kSlots x the largest array seen stay pinned
  void reserve(size_t bytes) {
    if (bytes <= slotBytes) return;
    if (slotBytes) hipCHECK(hipDeviceSynchronize());
    release();
    slotBytes = (std::max<size_t>(bytes, 512) + 255) & ~size_t(255);
    hipCHECK(hipHostMalloc((void**)&host, slotBytes * kSlots, hipHostMallocDefault));
    dev.resize(slotBytes * kSlots);
    for (int i = 0; i < kSlots; i++) hipCHECK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  }
  const void* push(const void* src, size_t bytes, hipStream_t stream) {
    reserve(bytes);
    const int s = next;
    next = (next + 1) % kSlots;
    if (used[s]) hipCHECK(hipEventSynchronize(ev[s]));
    std::memcpy(host + s * slotBytes, src, bytes);
    char* d = reinterpret_cast<char*>(dev.ptr) + s * slotBytes;
    hipCHECK(hipMemcpyAsync(d, host + s * slotBytes, bytes, hipMemcpyHostToDevice, stream));
    hipCHECK(hipEventRecord(ev[s], stream));
    used[s] = true;
    return d;
  }
};

// One pointer argument of an extension operation (hip_backend.h): `host` holds one device pointer per
// batch member.  A batch stages the array through the ring, once; a single call hands host[0] to the
// kernels directly.  at(q0): the members from q0 on.  A NULL array (an optional argument that was not
// given) stays the null DataRef.
template <typename T>
struct BatchPtrs {
  T* const* host = nullptr;
  T* const* dev = nullptr;
  BatchPtrs(PtrRing& ring, hipStream_t stream, T* const* host_, int64_t batch, bool single) : host(host_) {
    if (host && !single) dev = (T* const*)ring.push(host, batch * sizeof(T*), stream);
  }
  hipk::DataRef<T> at(int64_t q0) const {
    if (!host) return {nullptr, nullptr};
    return dev ? hipk::DataRef<T>{nullptr, dev + q0} : hipk::DataRef<T>{host[0], nullptr};
  }
};

struct HipSymElimCtx : SymElimCtx {
  int64_t lumpsBegin = 0, lumpsEnd = 0;
};

// launch recorder for the profiled mode (HIP events on the execution stream)
struct LaunchTimer {
  hipStream_t stream;
  HipKernelProfile* prof;
  struct Rec { int kind; hipEvent_t a, b; hipStream_t on; };
  vector<Rec> recs;
  LaunchTimer(hipStream_t s, HipKernelProfile* p) : stream(s), prof(p) {}
  // `on`: the stream the launch goes to (in-situ mode times the side-stream launches there)
  void begin(int kind, hipStream_t on = nullptr) {
    if (!prof) return;
    Rec r{kind, nullptr, nullptr, on ? on : stream};
    hipCHECK(hipEventCreate(&r.a));
    hipCHECK(hipEventCreate(&r.b));
    hipCHECK(hipEventRecord(r.a, r.on));
    recs.push_back(r);
  }
  void end() {
    if (!prof) return;
    hipCHECK(hipEventRecord(recs.back().b, recs.back().on));
  }
  void finish() {
    if (!prof) return;
    hipCHECK(hipStreamSynchronize(stream));  // (the side stream has been joined into it)
    // per class: sum of the launch durations, and the union of their intervals (device time
    // stamps relative to the first launch)
    vector<std::pair<float, float>> spans[kProfNumKinds];
    for (auto& r : recs) {
      float ms = 0, t0 = 0;
      hipCHECK(hipEventElapsedTime(&ms, r.a, r.b));
      if (&r != &recs.front()) hipCHECK(hipEventElapsedTime(&t0, recs.front().a, r.a));
      prof->ms[r.kind] += ms;
      prof->launches[r.kind]++;
      spans[r.kind].emplace_back(t0, t0 + ms);
    }
    for (int k = 0; k < kProfNumKinds; k++) {
      std::sort(spans[k].begin(), spans[k].end());
      float end = -1e30f;
      for (auto& sp : spans[k]) {
        if (sp.second <= end) continue;
        prof->busyMs[k] += sp.second - std::max(sp.first, end);
        end = sp.second;
      }
    }
    for (auto& r : recs) {
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
    recs.clear();
  }
};

// The auxiliary streams of the lookahead schedule are shared by every Solver of the process, one
// set per device, created on first use and kept for the life of the process.  HIP multiplexes its
// streams onto a handful of hardware queues (4 by default): with streams of their own, a second
// Solver's side streams landed on the queue of the execution stream and its lookahead work ran
// behind the chain instead of beside it (64 x GRID 17.4 instead of 14.5 ms, the fp32 BAL-1723 factor
// 26 instead of 19 ms, while another Solver was merely alive: tools/exp_order.py).  One factor() at a
// time per Solver is the contract (Solver.h); two Solvers factoring concurrently share these
// streams and are merely ordered on them.
struct SharedStreams {
  hipStream_t side = nullptr, due = nullptr;
  hipStream_t batch[3] = {nullptr, nullptr, nullptr};  // further parts of a batch factored as concurrent sub-batches (normal priority)
};
inline SharedStreams& sharedStreams() {
  static std::mutex mu;
  static std::map<int, SharedStreams> perDevice;
  int dev = 0;
  hipCHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  SharedStreams& st = perDevice[dev];
  if (!st.side) {
    int least = 0, greatest = 0;
    hipCHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    // lowest priority; neither stream priorities nor CU masks separate the bulk tiles from the
    // chain on this stack (hipExtStreamCreateWithCUMask is not honoured: a masked saturating kernel
    // ran on all 256 CUs, tools/throttle_probe.hip), what does is s_setprio inside the chain kernels
    hipCHECK(hipStreamCreateWithPriority(&st.side, hipStreamNonBlocking, least));
    // (highest priority for the due units: measured, no effect)
    hipCHECK(hipStreamCreateWithPriority(&st.due, hipStreamNonBlocking, least));
    for (hipStream_t& b : st.batch) hipCHECK(hipStreamCreateWithFlags(&b, hipStreamNonBlocking));
  }
  return st;
}

// per-op statistics of the per-op boundary (OpStat, Utils.h:48-121 of the reference): HIP events
// around the launches of one op, read back synchronously -- only while stats are enabled
struct OpTimer {
  OpStat& st;
  hipStream_t stream;
  hipEvent_t a = nullptr, b = nullptr;
  double s0, s1, s2;
  OpTimer(OpStat& st_, hipStream_t stream_, double s0_ = 0, double s1_ = 0, double s2_ = 0)
      : st(st_), stream(stream_), s0(s0_), s1(s1_), s2(s2_) {
    if (!st.enabled) return;
    hipCHECK(hipEventCreate(&a));
    hipCHECK(hipEventCreate(&b));
    hipCHECK(hipEventRecord(a, stream));
  }
  ~OpTimer() {
    if (!a) return;
    float ms = 0;
    if (hipEventRecord(b, stream) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
        hipEventElapsedTime(&ms, a, b) == hipSuccess) {
      st.add(ms * 1e-3, s0, s1, s2);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
};

// restores a flag on every exit (an exception from hipCHECK / launchLevels included)
struct FlagOff {
  bool& flag;
  const bool saved;
  explicit FlagOff(bool& f) : flag(f), saved(f) { flag = false; }
  ~FlagOff() { flag = saved; }
  FlagOff(const FlagOff&) = delete;
  FlagOff& operator=(const FlagOff&) = delete;
};


// ---- what a context keeps on the device, in groups that own their resources: resetting a group
// releases everything in it, and a new member is released with the rest (releaseDeviceState)

// events handed out in order and reused from call to call
struct EventPool {
  vector<hipEvent_t> all;
  size_t next = 0;
  EventPool() {}
  EventPool(const EventPool&) = delete;
  EventPool& operator=(const EventPool&) = delete;
  ~EventPool() {
    for (hipEvent_t e : all) (void)hipEventDestroy(e);
  }
  hipEvent_t take() {
    if (next == all.size()) {
      hipEvent_t e;
      hipCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      all.push_back(e);
    }
    return all[next++];
  }
};

// pinned host word a watchdog raises (persistent sweeps and tails), and its device alias
struct PinnedWord {
  unsigned* host = nullptr;
  unsigned* dev = nullptr;
  PinnedWord() {}
  PinnedWord(const PinnedWord&) = delete;
  PinnedWord& operator=(const PinnedWord&) = delete;
  ~PinnedWord() {
    if (host) (void)hipHostFree(host);
  }
};

// mirror of the skeleton (what SkelDev and deviceAccessor() point into)
struct SkelMirror {
  bool uploaded = false;
  DevBuf spanStart, spanToLump, lumpStart, spanOffsetInLump, chainColPtr, chainRowSpan, chainData,
      chainRowsTillEnd, boardColPtr, boardChainColOrd, permutation;
};

// plans, streams, events and the scratch of the factor launches
struct FactorState {
  std::map<std::tuple<int, int64_t, int64_t>, std::unique_ptr<DevPlan>> plans;
  SharedStreams* shared = nullptr;  // this device's auxiliary streams (streams())
  EventPool events;
  // scratch that outlives the per-call NumericCtx / SolveCtx objects (those are created and
  // destroyed around every factor() / solve(), Solver.cpp:176,223, while their kernels may still be
  // queued): sized on first use, only ever grown
  DevBuf dinvScratch, rawScratch, yieldBuf;
  DevBuf tailCtl, tailDinv;   // persistent tail (hip_tail_kernel.h): control words, inverted diagonal blocks
  PtrRing ptrRing;            // pointer arrays of batched calls (factor, solve and extension operations)
};

// scratch of the solve launches and the watchdog word of the persistent kernels
struct SolveState {
  // block solves through inverted diagonal blocks (denseLevels): the inverses of one solve call, and
  // per level list the panels whose diagonal blocks are inverted (uploaded once)
  DevBuf solveInvScratch;
  DevBuf solveWideBuf;        // [row][16] copy of the rows below an elimination range (hip_solve_wide.h)
  DevBuf sweepXchg;           // control words + exchange values of one denseLevels call
  DevBuf sweepTrace;          // developer aid (BSP_SWEEP_TRACE=1): clock stamps of the spines of the last sweep
  PinnedWord errWord;         // raised by a timed-out sweep or tail
  int sweepCapacity = 0;      // workgroups of a sweep launch that are resident at once (one per CU)
  size_t sweepMaxLds = 0;
  int sweepAttr[2] = {0, 0};  // per value size (8, 4): 0 not tried, 1 ready, -1 failed
  // (lump, row tile) lists of addMvFrom, per lump range
  std::map<std::pair<int64_t, int64_t>, std::pair<std::unique_ptr<DevBuf>, size_t>> addMvTileLists;
};

// selected-inversion plans and their scratch, work lists of the gradient kernels (hip_extensions.hip)
struct ExtensionState;
struct ExtensionStateDelete {
  void operator()(ExtensionState* p) const;
};

// back to a freshly constructed group: the members' destructors release what they own
template <typename G>
void resetGroup(G& g) {
  g.~G();
  new (&g) G();
}

struct HipSymbolicCtx : SymbolicCtx {
  const CoalescedBlockMatrixSkel& skel;
  vector<int64_t> permutation;
  vector<int64_t> sparseElimRanges;
  hipStream_t stream = nullptr;

  // ---- on the device (releaseDeviceState resets exactly these)
  SkelMirror mirror;
  FactorState fac;
  SolveState sol;
  std::unique_ptr<ExtensionState, ExtensionStateDelete> ext;  // built on first use

  // ---- device binding
  int device = -1;  // device of the first use (checkDevice)
  bool inPrepare = false;
  bool eagerOnly = false;  // so far only prepareDevice() has touched `device` (cleared by the first plan use)

  // ---- switches of the factor
  HipKernelProfile* profile = nullptr;
  bool profileInSitu = false;  // profile with the lookahead schedule left on (two streams)
  bool lookaheadEnabled = true;
  bool lazyPlan = false;  // HipBackendOptions::lazyPlan
  // LDS padding of side-stream launches: three bulk workgroups per CU, so that a chain workgroup
  // always finds a slot
  static constexpr unsigned bulkExtraLds = 6 * 1024, dueExtraLds = 6 * 1024;
  bool forcePerOp = false;  // TESTING: drive factor() through the per-op boundary
  // TESTING, fault injection (bsp_test_set_fault, include/baspacho_amd_testing.h; never read from the
  // environment): the sparse-elimination update is not launched, so the factor is wrong and the
  // full-size checks must notice
  bool faultDropElimUpdate = false;
  HipPlanOptions planOpts;     // the plan builder's switches (BSP_DUE_STREAM, BSP_BULK_AHEAD, ...)
  double lookaheadMinFlops = HipPlanHost::kMinDeferredFlopsPerFork;  // BSP_LOOKAHEAD_MIN_GF (0: side streams whenever a plan has lookahead units)
  bool potrfInTrsm = true;  // small multi-panel levels: potrf folded into the trsm launch (developer: BSP_POTRF_IN_TRSM=0)
  int64_t foldMaxTiles = 512;  // ... levels of at most this many row tiles x batch (developer: BSP_FOLD_MAX_TILES)
  bool splitK = true;       // split-K tile lists for small multi-panel levels (BSP_SPLIT_K=0: off)
  static constexpr int64_t splitKMaxWgs = 1024;  // ... launches of at most this many workgroups (a batch of 8: 2.26 = 2.26 ms at 1024, 2.48 at 4096)
  int subBatchMin = 16;     // batches of at least this many matrices are factored as concurrent sub-batches (BSP_SUB_BATCH_MIN; 0: never)
  int subBatchParts = 2;    // ... this many (BSP_SUB_BATCHES, at most 4, at least subBatchMin / 2 matrices each)
  int traceLaunchId = 0;  // ordinal of the chain-step launches (trace builds only)
  int tailFlags = 1;          // TailDesc::flags (BSP_TAIL_FLAGS)
#ifndef BSP_UPD_PREFETCH_MAX_WGS
#define BSP_UPD_PREFETCH_MAX_WGS 2048
#endif
  static constexpr int64_t updPrefetchMaxWgs = BSP_UPD_PREFETCH_MAX_WGS;  // updateTile<PREFETCH> for launches of up to this many workgroups

  // ---- switches of the solve
  bool blockSolve = true;   // wide lumps: triangular solves by outer block (BSP_BLOCK_SOLVE=0: by panel)
  uint64_t solveInvGen = 0;  // bumped by every launch that writes solveInvScratch
  bool solveInv = true;  // BSP_SOLVE_INV=0: the substitution kernels of rounds 1-2
  // persistent sweeps over wide lumps (hip_sweep_kernels.h, round 6)
  bool sweepEnabled = true;   // BSP_SOLVE_SWEEP=0: the multi-launch block path
  int sweepMinWidth = 768;    // runs of one-panel levels at least this wide (BSP_SWEEP_MIN_WIDTH)
  // ... and the narrowest run of columns it takes (ten right-hand sides, matrix-core sweep against the block path:
  // 2751 / 2814 columns +23 / +22 %, 6101 +7 %, 2442 +3 %; 7839 -8 %, 9756 -20 %; developer: BSP_SWEEP_MFMA_MIN_WIDTH)
  int sweepMfmaMinWidth = 7000;
  int sweepMfmaMinRhs = 8;    // right-hand sides from which the matrix-core sweep takes over (BAL-871: equal to the multi-launch path at 6, -5 % at 10, -10 % at 16; developer: BSP_SWEEP_MFMA_MIN)
  bool sweepBroken = false;   // a sweep timed out or cannot be launched here: multi-launch path for good
  int sweepFault = 0;         // TESTING (bsp_test_set_fault kind 2): spine of block 1 never publishes
  double sweepSpinLimitS = 2.0;  // watchdog: a spin that lasts longer aborts the launch
  bool solveWide = true;      // backward elimination pass with the right-hand sides across the lanes (hip_solve_wide.h)
  int solveWideMinRhs = 2;    // (developer: BSP_SOLVE_WIDE_MIN)
  size_t solveWideMaxBytes = (size_t)1 << 30;
  bool sweepTraceOn = false;

  // ---- switches of the extension operations
  int64_t selInvChunkCap = 0;          // TESTING: most matrices per selected-inversion chunk (0: no cap)

  HipRunCounters counters;  // (the two derived fields are filled in by hipBackendRunCounters)

  // `o`: the caller's switches with the environment already applied (backend_options.h)
  HipSymbolicCtx(const CoalescedBlockMatrixSkel& skel_, const vector<int64_t>& permutation_,
                 const HipBackendOptions& o);

  virtual void setSparseElimRanges(const vector<int64_t>& ranges) override;
  virtual void prepareFactor(int64_t upToLump) override;
  void releaseDeviceState();
  void prepareDevice(int64_t upToLump);
  virtual void setStream(void* s) override { stream = (hipStream_t)s; }
  void checkDevice();
  void uploadSkel();
  void ensureSkelOnDevice() {
    if (!mirror.uploaded) uploadSkel();
  }

  hipk::SkelDev skelDev() {
    ensureSkelOnDevice();
    hipk::SkelDev d;
    d.spanStart = mirror.spanStart.as<int64_t>();
    d.spanToLump = mirror.spanToLump.as<int64_t>();
    d.lumpStart = mirror.lumpStart.as<int64_t>();
    d.spanOffsetInLump = mirror.spanOffsetInLump.as<int64_t>();
    d.chainColPtr = mirror.chainColPtr.as<int64_t>();
    d.chainRowSpan = mirror.chainRowSpan.as<int64_t>();
    d.chainData = mirror.chainData.as<int64_t>();
    d.chainRowsTillEnd = mirror.chainRowsTillEnd.as<int64_t>();
    d.boardColPtr = mirror.boardColPtr.as<int64_t>();
    d.boardChainColOrd = mirror.boardChainColOrd.as<int64_t>();
    return d;
  }
  virtual PermutedCoalescedAccessor deviceAccessor() override;
  virtual SymElimCtxPtr prepareElimination(int64_t lumpsBegin, int64_t lumpsEnd) override;

  // ---- the call path of the extension operations (hip_backend.h) -----------------------------------
  // Every argument is a host array of one device pointer per batch member (BatchPtrs), staged in the
  // order the operation names them; the batch then runs in chunks of at most `chunk` members, one
  // after the other on the execution stream, a chunk being launches with gridDim.y = its members.
  template <typename T>
  BatchPtrs<T> stage(T* const* host, int64_t batch, bool single) {
    return BatchPtrs<T>(fac.ptrRing, stream, host, batch, single);
  }
  // run(q0, nm) enqueues the members q0 .. q0 + nm - 1
  template <typename F>
  void forChunks(int64_t batch, int64_t chunk, F&& run) {
    for (int64_t q0 = 0; q0 < batch; q0 += chunk) run(q0, (unsigned)std::min(chunk, batch - q0));
    hipCHECK(hipGetLastError());
  }
  // most members of one launch (gridDim.y)
  static constexpr int64_t kMaxGridY = 65535;
  DevPlan& planFor(const vector<int64_t>& ranges, int64_t startLump, int64_t upToLump, int tag);

  virtual NumericCtxBase* createNumericCtxForType(std::type_index tIdx, int64_t tempBufSize,
                                                  int batchSize) override;

  virtual SolveCtxBase* createSolveCtxForType(std::type_index tIdx, int nRHS,
                                              int batchSize) override;

  // side streams (shared, see sharedStreams) + event pool of the lookahead schedule
  // (resolved once per Solver, after checkDevice pinned its device: sharedStreams() takes a global
  //  mutex and asks for the current device, several times per level on a launch-bound path)
  SharedStreams& streams() {
    if (!fac.shared) {
      checkDevice();
      fac.shared = &sharedStreams();
    }
    return *fac.shared;
  }
  hipStream_t sideStream() { return streams().side; }
  // word of device memory through which the chain's potrf workgroup tells the bulk tiles which CU
  // it runs on (cooperative CU yield, hip_kernels.h)
  unsigned* yieldWord() {
    if (!fac.yieldBuf.ptr) {
      const size_t bytes = 256;  // word 0: the potrf workgroup's CU
      fac.yieldBuf.resize(bytes);
      hipCHECK(hipMemset(fac.yieldBuf.ptr, 0, bytes));
    }
    return reinterpret_cast<unsigned*>(fac.yieldBuf.ptr);
  }
  hipStream_t dueSideStream() { return streams().due; }
  hipEvent_t eventFromPool() { return fac.events.take(); }
  void resetEventPool() { fac.events.next = 0; }
  // a timed-out persistent launch (solve sweep, factor tail) is reported ONCE, by the next factor()
  // or solve() on this Solver; the persistent kernels are then retired for good
  void checkAsyncError() {
    if (sol.errWord.host && *reinterpret_cast<volatile unsigned*>(sol.errWord.host) != 0u) {
      *reinterpret_cast<volatile unsigned*>(sol.errWord.host) = 0u;
      sweepBroken = true;
      counters.sweepTimeouts++;
      if (planOpts.tailBlocks > 0) {
        (void)hipDeviceSynchronize();  // (nothing of the old plans may still be queued)
        planOpts.tailBlocks = 0;
        fac.plans.clear();
      }
      throw std::runtime_error(
          "HIP backend: a persistent launch (solve sweep / factor tail) of an EARLIER call on this "
          "Solver timed out (watchdog); the result of that call is invalid.  The persistent kernels "
          "are retired for this Solver: it takes the multi-launch paths from now on");
    }
  }
  bool sweepUsable() {
    checkAsyncError();
    return sweepEnabled && !sweepBroken && solveInv && blockSolve;
  }
  long long* tailTrace();
  hipError_t allocAsyncErrWord();
  unsigned* asyncErrWord();
};

// hip_factor.hip / hip_solve.hip: the contexts of one factor() / solve() call
NumericCtxBase* createHipNumericCtx(HipSymbolicCtx& sym, std::type_index tIdx, int64_t tempBufSize, int batchSize);
SolveCtxBase* createHipSolveCtx(HipSymbolicCtx& sym, std::type_index tIdx, int nRHS, int batchSize);
// hip_factor.hip: loads the factor kernels' code object (one empty launch on `stream`)
void launchFactorWarmup(hipStream_t stream);

}  // namespace hipb
}  // namespace BaSpaCho
