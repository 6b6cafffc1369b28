// MI355X backend: the symbolic context (options, device binding, skeleton mirror, plan cache,
// streams and events, watchdog word), the Ops factory, and the host-only queries and switches of
// hip_backend.h.  The launch paths live beside it: hip_factor.hip (NumericCtx), hip_solve.hip
// (SolveCtx), hip_extensions.hip (selected inversion, gradients, adjoints, assembly).
// Takes the place of baspacho/baspacho/MatOpsCuda.cu (CudaSymbolicCtx :56-143, CudaNumericCtx
// :408-604, batched :605-725) without cuBLAS/cuSOLVER, per-op syncs, per-call allocations or
// per-lump host->device table uploads.
#include <new>

#include "hip_context.h"

namespace BaSpaCho {

using std::vector;
using namespace hipb;

// `o`: the caller's switches with the environment already applied (backend_options.h)
HipSymbolicCtx::HipSymbolicCtx(const CoalescedBlockMatrixSkel& skel_, const vector<int64_t>& permutation_,
                               const HipBackendOptions& o)
    : skel(skel_), permutation(permutation_) {
  lookaheadEnabled = HipBackendOptions::on(o.lookahead, true);
  blockSolve = HipBackendOptions::on(o.blockSolve, true);
  solveInv = HipBackendOptions::on(o.solveInv, true);
  if (o.subBatchMin >= 0) subBatchMin = o.subBatchMin == 0 ? INT32_MAX : std::max(2, o.subBatchMin);
  if (o.subBatches >= 0) subBatchParts = std::max(2, o.subBatches);
  splitK = HipBackendOptions::on(o.splitK, true);
  sweepEnabled = HipBackendOptions::on(o.solveSweep, true);
  solveWide = HipBackendOptions::on(o.solveWide, true);
  if (o.sweepMinWidth >= 0) sweepMinWidth = std::max(1, o.sweepMinWidth);
  lazyPlan = HipBackendOptions::on(o.lazyPlan, false);
  if (!std::isnan(o.lookaheadMinGF)) lookaheadMinFlops = 1e9 * o.lookaheadMinGF;
  // the plan builder's switches: handed to every buildHipPlan call and recorded in the plan;
  // launchLevels takes dueStream from the plan it runs
  planOpts.dueStream = HipBackendOptions::on(o.dueStream, planOpts.dueStream);
  if (o.gatherMaxPairs >= 0) planOpts.gatherMaxPairs = std::max(8, o.gatherMaxPairs);
  if (!std::isnan(o.bulkAhead)) planOpts.bulkAhead = o.bulkAhead;
  if (o.tailBlocks >= 0) planOpts.tailBlocks = o.tailBlocks;
  planOpts.applyDeveloperEnv();
  // developer aids and experiment parameters that are not options of the product
  if (const char* e = std::getenv("BSP_TAIL_FLAGS")) tailFlags = std::atoi(e);
  if (const char* e = std::getenv("BSP_SWEEP_TRACE")) sweepTraceOn = e[0] != '0';
  if (const char* e = std::getenv("BSP_SWEEP_MFMA_MIN")) sweepMfmaMinRhs = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("BSP_SWEEP_MFMA_MIN_WIDTH")) sweepMfmaMinWidth = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("BSP_SOLVE_WIDE_MIN")) solveWideMinRhs = std::max(2, std::atoi(e));
  if (const char* e = std::getenv("BSP_POTRF_IN_TRSM")) potrfInTrsm = e[0] != '0';
  if (const char* e = std::getenv("BSP_FOLD_MAX_TILES")) foldMaxTiles = std::min<int64_t>(kFoldMaxTiles, std::max(1, std::atoi(e)));
}

void HipSymbolicCtx::setSparseElimRanges(const vector<int64_t>& ranges) {
  sparseElimRanges = ranges;
  fac.plans.clear();
}

void HipSymbolicCtx::prepareFactor(int64_t upToLump) {
  try {
    prepareDevice(upToLump);
  } catch (const std::exception&) {
    // (eager preparation is an optimisation: whatever it could not do happens -- and fails
    //  loudly, if it has to -- in the first factor().  Nothing of the eager state has been handed
    //  out: release ALL of it and forget the device, so that a first real use on another device
    //  binds there as the lazy path of rounds 1-3 did)
    (void)hipGetLastError();
    releaseDeviceState();
    device = -1;
    eagerOnly = false;
    inPrepare = false;
  }
}

// everything this context has put on the GPU (a device buffer is freed on whatever device is
// current; events and plans likewise)
void HipSymbolicCtx::releaseDeviceState() {
  resetGroup(fac);
  resetGroup(sol);
  resetGroup(mirror);
  ext.reset();
}

// The reference builds its SymbolicCtx and every SymElimCtx in the Solver constructor
// (Solver.cpp:24-40), so that its first factor() costs what every later one does.  Same here: when
// a GPU is visible at construction, the full-range factor plan is built and uploaded, the skeleton
// mirrors, scratch buffers, auxiliary streams and the event pool are created and the factor kernels'
// code object is loaded (one empty launch; the solve and extension kernels load with their first call) -- all on the device that is current NOW.  A Solver whose
// first real use happens with another device current re-binds there (nothing of the eager state
// has been handed out yet); plans of partial ranges stay lazy.  Without a GPU (symbolic analysis
// on a host-only box) nothing happens here.
void HipSymbolicCtx::prepareDevice(int64_t upToLump) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return;
  }
  if (lazyPlan) return;  // (A/B: the lazy behaviour of rounds 1-3)
  struct Scope {
    bool& f;
    explicit Scope(bool& f_) : f(f_) { f = true; }
    ~Scope() { f = false; }
  } scope(inPrepare);
  if (upToLump <= 0) return;
  DevPlan& plan = planFor(sparseElimRanges, 0, upToLump, /*tag=*/0);
  ensureSkelOnDevice();
  (void)streams();
  (void)yieldWord();
  // scratch of the chain kernels, sized for one fp64 matrix (grown later for batches)
  fac.dinvScratch.resize((size_t)hipk::kDinvBatchStride * sizeof(double));
  if (plan.host.maxChainRows > 0) {
    fac.rawScratch.resize((size_t)2 * plan.host.maxChainRows * kTile * sizeof(double));
  }
  const size_t wantEvents = 8 + 4 * (size_t)plan.host.numForkLevels;
  while (fac.events.all.size() < wantEvents) {
    hipEvent_t e;
    hipCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    fac.events.all.push_back(e);
  }
  // code object load: one empty launch on a private non-blocking stream (the context's own
  // stream is the legacy default stream at construction: a launch + sync there would also wait for
  // every blocking stream of the process -- PyTorch's included -- and is illegal during a capture)
  {
    hipStream_t warm = nullptr;
    hipCHECK(hipStreamCreateWithFlags(&warm, hipStreamNonBlocking));
    launchFactorWarmup(warm);
    const hipError_t werr = hipStreamSynchronize(warm);
    (void)hipStreamDestroy(warm);
    hipCHECK(werr);
  }
  eagerOnly = true;
}

// Everything a Solver puts on the GPU (skeleton mirrors, plans, scratch, streams, events) lives
// on the device that was current at its first use; later calls must run with that device current.
void HipSymbolicCtx::checkDevice() {
  int cur = -1;
  hipCHECK(hipGetDevice(&cur));
  if (device < 0) device = cur;
  if (cur != device && eagerOnly) {
    // only the constructor's eager state lives on `device`: move to the device of the first use
    releaseDeviceState();
    device = cur;
  }
  if (!inPrepare) eagerOnly = false;
  if (cur != device) {
    throw std::runtime_error("HIP backend: this Solver was first used on device " +
                             std::to_string(device) + " but the current device is " +
                             std::to_string(cur) + " (make its device current before the call)");
  }
}

void HipSymbolicCtx::uploadSkel() {
  checkDevice();
  mirror.spanStart.upload(skel.spanStart);
  mirror.spanToLump.upload(skel.spanToLump);
  mirror.lumpStart.upload(skel.lumpStart);
  mirror.spanOffsetInLump.upload(skel.spanOffsetInLump);
  mirror.chainColPtr.upload(skel.chainColPtr);
  mirror.chainRowSpan.upload(skel.chainRowSpan);
  mirror.chainData.upload(skel.chainData);
  mirror.chainRowsTillEnd.upload(skel.chainRowsTillEnd);
  mirror.boardColPtr.upload(skel.boardColPtr);
  mirror.boardChainColOrd.upload(skel.boardChainColOrd);
  mirror.permutation.upload(permutation);
  mirror.uploaded = true;
}

PermutedCoalescedAccessor HipSymbolicCtx::deviceAccessor() {
  ensureSkelOnDevice();
  PermutedCoalescedAccessor acc;
  acc.init(mirror.spanStart.as<int64_t>(), mirror.spanToLump.as<int64_t>(), mirror.lumpStart.as<int64_t>(),
           mirror.spanOffsetInLump.as<int64_t>(), mirror.chainColPtr.as<int64_t>(),
           mirror.chainRowSpan.as<int64_t>(), mirror.chainData.as<int64_t>(), mirror.permutation.as<int64_t>());
  return acc;
}

SymElimCtxPtr HipSymbolicCtx::prepareElimination(int64_t lumpsBegin, int64_t lumpsEnd) {
  HipSymElimCtx* e = new HipSymElimCtx;
  e->lumpsBegin = lumpsBegin;
  e->lumpsEnd = lumpsEnd;
  return SymElimCtxPtr(e);
}

// plan of a fused factor over lumps [startLump, upToLump), built and uploaded on first use
// tag 0: factor() / solve(); tag 1: one elimination range; tag 2: factor() of a BATCH when plan 0 has a
// persistent tail -- the same plan without it.  The tail is a latency device for ONE matrix: in a batch
// the chain steps of the matrices already run side by side, and batch x roles exceed what is resident
// (batch of 8 GRID 82x82 2.23 -> 2.35 ms with it; the reference's FLAT families at batch 16 +22..+36 % per
// matrix, profiles/r06_tail_batches.txt)
DevPlan& HipSymbolicCtx::planFor(const vector<int64_t>& ranges, int64_t startLump, int64_t upToLump, int tag) {
  checkDevice();
  auto key = std::make_tuple(tag, startLump, upToLump);
  auto it = fac.plans.find(key);
  if (it == fac.plans.end()) {
    std::unique_ptr<DevPlan> p(new DevPlan);
    HipPlanOptions po = planOpts;
    if (tag == 2) po.tailBlocks = 0;
    p->host = buildHipPlan(skel, ranges, startLump, upToLump, po);
    p->upload();
    it = fac.plans.emplace(key, std::move(p)).first;
  }
  return *it->second;
}

NumericCtxBase* HipSymbolicCtx::createNumericCtxForType(std::type_index tIdx, int64_t tempSize, int batch) {
  return createHipNumericCtx(*this, tIdx, tempSize, batch);
}

SolveCtxBase* HipSymbolicCtx::createSolveCtxForType(std::type_index tIdx, int nRHS, int batch) {
  return createHipSolveCtx(*this, tIdx, nRHS, batch);
}

long long* HipSymbolicCtx::tailTrace() {  // developer aid (BSP_SWEEP_TRACE=1): the spines' clock stamps
  if (!sweepTraceOn) return nullptr;
  if (!sol.sweepTrace.ptr) {
    sol.sweepTrace.resize(8 * 4096 * sizeof(long long));
    hipCHECK(hipMemset(sol.sweepTrace.ptr, 0, 8 * 4096 * sizeof(long long)));
  }
  return reinterpret_cast<long long*>(sol.sweepTrace.ptr);
}
// pinned host word a watchdog raises (persistent sweeps and tails), and its device alias: allocated
// on first use.  An error of the runtime is returned, and nothing is kept then
hipError_t HipSymbolicCtx::allocAsyncErrWord() {
  if (sol.errWord.host) return hipSuccess;
  void *hp = nullptr, *dp = nullptr;
  hipError_t e = hipHostMalloc(&hp, 64, hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, hp, 0);
  if (e != hipSuccess) {
    if (hp) (void)hipHostFree(hp);
    return e;
  }
  sol.errWord.host = reinterpret_cast<unsigned*>(hp);
  *sol.errWord.host = 0u;
  sol.errWord.dev = reinterpret_cast<unsigned*>(dp);
  return hipSuccess;
}
unsigned* HipSymbolicCtx::asyncErrWord() {
  hipCHECK(allocAsyncErrWord());
  return sol.errWord.dev;
}

namespace {

struct HipOps : Ops {
  explicit HipOps(const HipBackendOptions& o) : options(o) {}
  virtual SymbolicCtxPtr createSymbolicCtx(const CoalescedBlockMatrixSkel& skel,
                                           const vector<int64_t>& permutation) override {
    return SymbolicCtxPtr(new HipSymbolicCtx(skel, permutation, options));
  }
  HipBackendOptions options;
};

}  // namespace

OpsPtr hipOps(const HipBackendOptions* options) {
  if (options) return OpsPtr(new HipOps(*options));
  HipBackendOptions o;  // (callers that build a Solver from a skeleton: defaults + environment)
  o.applyEnv();
  return OpsPtr(new HipOps(o));
}

void hipBackendForcePerOp(SymbolicCtx& sym, bool on) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  h->forcePerOp = on;
}

std::vector<int64_t> hipBackendPlanLevels(SymbolicCtx& sym, int64_t startLump, int64_t upToLump) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  HipPlanHost p = buildHipPlan(h->skel, h->sparseElimRanges, startLump, upToLump, h->planOpts);
  std::vector<int64_t> out;
  auto emit = [&](const vector<LevelRange>& levels, int64_t range) {
    for (const LevelRange& lr : levels) {
      int64_t maxNb = 0, maxRows = 0, sumRows = 0;
      for (int64_t q = lr.panelBegin; q < lr.panelEnd; q++) {
        const PanelDesc& pd = p.panels[p.levelPanels[q]];
        maxNb = std::max<int64_t>(maxNb, pd.nb);
        maxRows = std::max<int64_t>(maxRows, pd.rowsBelow);
        sumRows += pd.rowsBelow;
      }
      const int64_t row[8] = {range, lr.panelEnd - lr.panelBegin, maxNb, maxRows, lr.trsmEnd - lr.trsmBegin,
                              lr.updEnd - lr.updBegin, lr.defEnd - lr.defBegin, sumRows};
      out.insert(out.end(), row, row + 8);
    }
  };
  for (size_t r = 0; r < p.elimRanges.size(); r++) emit(p.elimRanges[r].bigLevels, (int64_t)r);
  emit(p.levels, -1);
  return out;
}

std::vector<int64_t> hipBackendLaunchTableRecords(SymbolicCtx& sym) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  const HipPlanHost p = buildHipPlan(h->skel, h->sparseElimRanges, 0, h->skel.numLumps(), h->planOpts);
  const LaunchTables t = buildLaunchTables(p);
  int64_t numLevels = (int64_t)p.levels.size();
  for (const ElimRangePlan& er : p.elimRanges) numLevels += (int64_t)er.bigLevels.size();
  std::vector<int64_t> out = {numLevels, (int64_t)p.levels.size(), (int64_t)p.levelPanels.size(),
                              (int64_t)p.trsmTasks.size(), (int64_t)p.updTasks.size(),
                              (int64_t)t.levelPanelDescs.size(), (int64_t)t.trsmTasksFat.size(),
                              (int64_t)t.updTasksFat.size(), (int64_t)t.updTasksWide.size(),
                              (int64_t)t.slowPrefix.size(), (int64_t)t.updTasksSplit.size(),
                              (int64_t)t.splitRange.size(), (int64_t)t.foldRank.size(), (int64_t)t.foldTiles.size(),
                              (int64_t)t.foldPanelEnd.size(), (int64_t)t.foldDescs.size()};
  auto levels = [&](const vector<LevelRange>& ls, int64_t range) {
    for (const LevelRange& lr : ls) {
      out.insert(out.end(), {range, (int64_t)lr.tail, (int64_t)lr.directPanel, lr.panelBegin, lr.panelEnd, lr.trsmBegin,
                             lr.trsmEnd, lr.updBegin, lr.updEnd});
    }
  };
  for (size_t r = 0; r < p.elimRanges.size(); r++) levels(p.elimRanges[r].bigLevels, (int64_t)r);
  levels(p.levels, -1);
  auto panels = [&](const vector<PanelDesc>& ps) {
    for (const PanelDesc& d : ps) {
      out.insert(out.end(), {d.diagOff, (int64_t)d.lda, (int64_t)d.nb, (int64_t)d.rowsBelow, (int64_t)d.nRest,
                             (int64_t)d.lumpRowBase, (int64_t)d.lump, (int64_t)d.vecOff});
    }
  };
  auto wide = [&](const vector<UpdTaskWide>& ws) {
    for (const UpdTaskWide& w : ws) {
      out.insert(out.end(), {w.srcOff, w.tgtBase, w.chainTabPtr, (int64_t)w.lda, (int64_t)w.K, (int64_t)w.rowsBelow,
                             (int64_t)w.nRest, (int64_t)w.lumpRowBase, (int64_t)w.kind, (int64_t)w.segEnd,
                             (int64_t)w.tgtStride, (int64_t)w.firstChainOrd, (int64_t)w.rowMin, (int64_t)w.rowTile,
                             (int64_t)w.colTile, (int64_t)w.atomic});
    }
  };
  panels(t.levelPanelDescs);
  for (const TrsmTaskFat& f : t.trsmTasksFat) {
    out.insert(out.end(), {f.diagOff, (int64_t)f.lda, (int64_t)f.nb, (int64_t)f.rowsBelow, (int64_t)f.rowTile});
  }
  for (const UpdTaskFat& f : t.updTasksFat) {
    out.insert(out.end(), {f.srcOff, f.tgtBase, (int64_t)f.lda, (int64_t)f.K, (int64_t)f.rowsBelow, (int64_t)f.segEnd,
                           (int64_t)f.rowTile, (int64_t)f.colTile, (int64_t)f.tgtStride, (int64_t)f.rowMin,
                           (int64_t)f.atomic, (int64_t)f.fast});
  }
  wide(t.updTasksWide);
  out.insert(out.end(), t.slowPrefix.begin(), t.slowPrefix.end());
  wide(t.updTasksSplit);
  for (const auto& sr : t.splitRange) out.insert(out.end(), {sr.first, sr.second.first, sr.second.second});
  out.insert(out.end(), t.foldRank.begin(), t.foldRank.end());
  out.insert(out.end(), t.foldTiles.begin(), t.foldTiles.end());
  out.insert(out.end(), t.foldPanelEnd.begin(), t.foldPanelEnd.end());
  panels(t.foldDescs);
  return out;
}

std::vector<int64_t> hipBackendSolveScheduleRecords(SymbolicCtx& sym, bool withSweeps, bool blockSolve, bool inverses,
                                                    int sweepMinWidth) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  const HipPlanHost p = buildHipPlan(h->skel, h->sparseElimRanges, 0, h->skel.numLumps(), h->planOpts);
  const SolveSchedule s = buildSolveSchedule(p, p.levels, {withSweeps, blockSolve, inverses, sweepMinWidth});
  std::vector<int64_t> out = {(int64_t)p.levels.size(), (int64_t)s.items.size(), (int64_t)s.invPanels.size(),
                              (int64_t)s.numSweeps, s.sweepInstStride, s.maxSweepWgs, s.maxSweepWgsM,
                              (int64_t)s.maxSweepW, (int64_t)s.maxSweepBelow};
  auto panel = [&](const PanelDesc& d) {
    out.insert(out.end(), {(int64_t)d.lump, (int64_t)(d.lda - d.nRest - d.nb), (int64_t)d.nb, (int64_t)d.rowsBelow});
  };
  for (const LevelRange& lr : p.levels) {
    out.push_back(lr.panelEnd - lr.panelBegin);
    if (lr.directPanel >= 0) {
      panel(p.panels[lr.directPanel]);
    } else {
      out.insert(out.end(), {-1, -1, -1, -1});
    }
  }
  for (const SolveSchedItem& it : s.items) {
    out.insert(out.end(), {(int64_t)it.kind, (int64_t)it.slot, it.l, it.e, (int64_t)it.sweep.w, (int64_t)it.sweep.nBlocks,
                           (int64_t)it.sweep.rowsBelow, (int64_t)it.sweep.invSlot, (int64_t)it.sweep.xchgOff,
                           (int64_t)it.sweepFwdWgs, (int64_t)it.sweepBwdWgs});
  }
  for (const PanelDesc& d : s.invPanels) panel(d);
  return out;
}

void hipBackendSetFault(SymbolicCtx& sym, int kind) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  h->faultDropElimUpdate = kind == 1;
  // kind 2: the spine of block 1 of every persistent solve sweep never publishes its x, with the
  // watchdog set to 50 ms: the launch must end by itself and the NEXT solve must report it
  h->sweepFault = kind == 2 ? 2 : 0;
  h->sweepSpinLimitS = kind == 2 ? 0.05 : 2.0;
}

HipRunCounters hipBackendRunCounters(SymbolicCtx& sym) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  HipRunCounters c = h->counters;
  c.sweepsRetired = h->sweepBroken ? 1 : 0;
  c.sweepErrorPending = (h->sol.errWord.host && *reinterpret_cast<volatile unsigned*>(h->sol.errWord.host)) ? 1 : 0;
  return c;
}

void hipBackendSetProfile(SymbolicCtx& sym, HipKernelProfile* prof, bool inSitu) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  h->profile = prof;
  h->profileInSitu = prof != nullptr && inSitu;
}

HipPlanStats hipBackendPlanStats(SymbolicCtx& sym, int64_t startLump, int64_t upToLump) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  // host-only: does not touch the device
  HipPlanHost p = buildHipPlan(h->skel, h->sparseElimRanges, startLump, upToLump, h->planOpts);
  HipPlanStats s;
  s.flops = p.flops;
  s.updElems = p.updElems;
  s.updFlops = p.updFlops;
  s.elimPairElems = p.elimPairElems;
  s.elimPairFlops = p.elimPairFlops;
  s.elimColElems = p.elimColElems;
  s.updFlopsDirect = p.updFlopsDirect;
  s.elimPairOperandElems = p.elimPairOperandElems;
  s.elimTargetElems = p.elimTargetElems;
  s.trsmFlops = p.trsmFlops;
  s.potrfFlops = p.potrfFlops;
  s.trsmFlopsMerged = p.trsmFlopsMerged;
  s.potrfFlopsFused = p.potrfFlopsFused;
  s.numLaunches = p.numLaunches;
  s.numLevels = (int64_t)p.levels.size();
  s.numPanels = (int64_t)p.panels.size();
  s.numSegs = (int64_t)p.segs.size();
  s.numUpdTasks = (int64_t)p.updTasks.size();
  s.numTrsmTasks = (int64_t)p.trsmTasks.size();
  s.chainTabEntries = (int64_t)p.chainOffTab.size();
  s.maxPanelsInLevel = p.maxPanelsInLevel;
  int64_t atomicTasks = 0;
  for (auto& t : p.updTasks) atomicTasks += t.atomic ? 1 : 0;
  s.numAtomicUpdTasks = atomicTasks;
  s.numForkLevels = p.numForkLevels;
  s.deferredFlops = p.deferredFlops;
  s.tailUpdFlops = p.tailUpdFlops;
  for (const LevelRange& lr : p.levels) s.numTailPanels += lr.tail ? 1 : 0;
  return s;
}

}  // namespace BaSpaCho
