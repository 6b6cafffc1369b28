// MI355X backend, the factor launch path: NumericCtx implemented with the hand-written HIP kernels
// of hip_kernels.h / hip_tail_kernel.h and the level-scheduled device plan of hip_plan.h.
#include <atomic>

#include "hip_context.h"
#include "hip_kernels.h"
#include "hip_tail_kernel.h"

namespace BaSpaCho {

using std::vector;
using namespace hipb;

namespace {

template <typename T>
struct HipNumericCtx : NumericCtx<T> {
  using BT = BaseType<T>;

  HipNumericCtx(HipSymbolicCtx& sym_, int batchSize_, int64_t tempBufSize_)
      : sym(sym_), batchSize(batchSize_), tempBufSize(std::max<int64_t>(tempBufSize_, 1)) {}

  // single matrix: pointer by value; batch: the device-pointer array is uploaded once per call
  hipk::DataRef<BT> makeRef(T* data);

  // extraLds: dynamic LDS requested on top of the kernel's static 35 KB.  Bulk (deferred) launches
  // ask for 6 KB so that only THREE of their workgroups fit on a CU (3 x 41 KB), leaving 37 KB for
  // a workgroup of the critical-path kernels (trsm needs 33.5 KB); with four resident bulk
  // workgroups the trsm of the next panel was starved for the whole bulk update (273 us vs 17 us).
  // atomicMask: which bits of a task's `atomic` field count (bit 1 = "launches of two side streams
  // may meet": only in due-stream mode)
  void launchUpdate(DevPlan& plan, int64_t begin, int64_t end, hipk::DataRef<BT> ref,
                    hipStream_t stream, BT* altTarget = nullptr, int64_t altStride = 0,
                    unsigned extraLds = 0, int atomicMask = 1) {
    if (altTarget == nullptr && end < (int64_t)plan.slowPrefix.size() &&
        plan.slowPrefix[end] == plan.slowPrefix[begin]) {
      // (32 KB of static LDS instead of updateTile's 34.8: 3 KB more padding keeps it at three
      //  workgroups per CU next to a chain workgroup)
      const unsigned pad = extraLds ? extraLds + 3072 : 0;
      // (cooperative CU yield, hip_kernels.h: side-stream launches of a single matrix only)
      const unsigned* yf = (extraLds && batchSize == 1) ? sym.yieldWord() : nullptr;
      hipk::updateTileBulk<BT><<<dim3((unsigned)(end - begin), (unsigned)batchSize), 256, pad,
                                stream>>>(plan.updTasksFat.as<UpdTaskFat>() + begin, ref, yf, atomicMask);
      return;
    }
    // (launches of at most ~2 rounds of workgroups: the latency-bound variant, hip_kernels.h)
    const int64_t wgs = (end - begin) * (int64_t)batchSize;
    const bool few = wgs <= sym.updPrefetchMaxWgs;
    auto kern = few ? hipk::updateTile<BT, true> : hipk::updateTile<BT, false>;
    // (Asking for enough dynamic LDS that only ceil(workgroups / CUs) of a small launch fit on a CU,
    //  in case the dispatcher packs them four to a CU: no effect at batch 1 / 8 / 64 -- it does not.)
    kern<<<dim3((unsigned)(end - begin), (unsigned)batchSize), 256, extraLds, stream>>>(
        plan.updTasksWide.as<UpdTaskWide>() + begin,
        plan.chainOffTab.as<int64_t>(), plan.rowChain.as<int32_t>(), plan.rowLocal.as<int32_t>(),
        plan.rowColOff.as<int32_t>(), ref, altTarget, altStride, atomicMask);
  }

  // One level = potrf -> trsm -> update on the execution stream.  Deferred (lookahead) tiles go to
  // the side stream after the level's trsm and are joined back by events where the plan says so.
  // (profiled runs serialise the launches on the execution stream, unless the in-situ mode asks
  //  for the real multi-stream schedule with every launch timed on the stream it runs on)
  bool lookaheadOn() const {
    return (sym.profile == nullptr || sym.profileInSitu) && sym.lookaheadEnabled;
  }

  void launchLevels(DevPlan& plan, const vector<LevelRange>& levels, hipk::DataRef<BT> ref,
                    LaunchTimer& timer) {
    const dim3 gy(1, (unsigned)batchSize, 1);
    // (side streams only when the lookahead units are worth their forks, HipPlanHost::lookaheadPays;
    //  otherwise the same launches go in line)
    const bool lookahead = lookaheadOn() && plan.host.lookaheadPays(batchSize, sym.lookaheadMinFlops);
    vector<hipEvent_t> defDone(levels.size(), nullptr);  // due units of a level complete
    vector<hipEvent_t> optDone(levels.size(), nullptr);  // ... its optional units (due-stream mode)
    // (fp32: its atomics cost more than the second stream returns -- BAL-871 5.86 against 5.22 ms,
    //  BAL-1723 20.5 against 18.8 -- so single-precision calls keep the one-side-stream order, and
    //  the tasks' "two streams may meet" bit is masked off)
    const bool dueStream = plan.host.opts.dueStream && sizeof(BT) == 8;
    const int sideMask = dueStream ? 3 : 1;
    // levels whose potrf is folded into their trsm launch in THIS call (DevPlan::foldRank): the first
    // nFold levels of the plan's order by row tiles
    int64_t nFold = 0;
    if (sym.potrfInTrsm && &levels == &plan.host.levels) {
      while (nFold < (int64_t)plan.foldTiles.size() &&
             plan.foldTiles[nFold] * (int64_t)batchSize <= sym.foldMaxTiles) {
        nFold++;
      }
    }
    // fork level of the same lump's previous block (-1: none)
    auto prevFork = [&](int64_t f) -> int64_t { return f >= 0 ? levels[f].waitDefLevel : -1; };
    auto waitDeferred = [&](int64_t f) {
      // everything the side streams owe to the column block this level is about to touch
      if (f < 0 || !defDone[f]) return;
      hipCHECK(hipStreamWaitEvent(sym.stream, defDone[f], 0));
      const int64_t pf = prevFork(f);
      if (dueStream && pf >= 0 && optDone[pf]) hipCHECK(hipStreamWaitEvent(sym.stream, optDone[pf], 0));
    };
    bool potrfFused = false;  // this level's potrf ran inside the previous level's update launch
    bool sideUsed = false, dueUsed = false;
    // inverted diagonal blocks of the chain panels: written by a panel's potrf, read by its trsm
    // (two slots per matrix, alternating from panel to panel)
    // (a batch factored as concurrent sub-batches, factorRange: every sub-batch its own slice)
    const int64_t scratchBatch = std::max<int64_t>(batchSize, subBatchTotal);
    sym.fac.dinvScratch.resize((size_t)scratchBatch * hipk::kDinvBatchStride * sizeof(BT));
    BT* dinvBase = const_cast<BT*>(sym.fac.dinvScratch.as<BT>()) + (size_t)subBatchBase * hipk::kDinvBatchStride;
    int dinvSlot = 0;  // slot of the current level's panel
    // staging buffer of the chain (chainStep): unsolved rows of the current / next panel
    const int64_t rawSlot = plan.host.maxChainRows * kTile;
    BT* rawBase = nullptr;
    if (rawSlot > 0) {
      sym.fac.rawScratch.resize((size_t)scratchBatch * 2 * rawSlot * sizeof(BT));
      rawBase = const_cast<BT*>(sym.fac.rawScratch.as<BT>()) + (size_t)subBatchBase * 2 * rawSlot;
    }
    bool rawValid = false;  // the previous level staged this level's panel rows
    // early tile-(0,0) updates of the next outer block (LevelRange::extraDiag): how many panels of
    // the current block have applied theirs, in order -- the block-last step's potrf workgroup
    // applies the rest from memory
    int extraApplied = 0;
    bool extraBroken = false;
    hipEvent_t lastOpt = nullptr;  // the most recent optional lookahead launch (side stream)
    for (size_t li = 0; li < levels.size(); li++) {
      const LevelRange& lr = levels[li];
      const unsigned nP = (unsigned)(lr.panelEnd - lr.panelBegin);
      const unsigned nT = (unsigned)(lr.trsmEnd - lr.trsmBegin);
      const bool direct = lr.directPanel >= 0;
      if (lr.tail) {
        if (lr.tail == 1) {
          // PERSISTENT TAIL (hip_tail_kernel.h): everything the lookahead streams still owe to these
          // columns first, then one launch for all the panels of the tail
          auto joinStream = [&](hipStream_t st) {
            hipEvent_t e = sym.eventFromPool();
            hipCHECK(hipEventRecord(e, st));
            hipCHECK(hipStreamWaitEvent(sym.stream, e, 0));
          };
          if (sideUsed) joinStream(sym.sideStream());
          if (dueUsed) joinStream(sym.dueSideStream());
          sideUsed = dueUsed = false;
          const PanelDesc& p0 = plan.host.panels[lr.directPanel];
          hipk::TailDesc td;
          td.diagOff = p0.diagOff;
          td.lda = p0.lda;
          td.K = p0.nb + p0.nRest;
          td.nP = (td.K + kTile - 1) / kTile;
          td.ctlStride = hipk::tailCtlWords(td.nP);
          td.flags = sym.tailFlags;
          td.pad = 0;
          BASPACHO_CHECK_EQ(td.nP, lr.tailPanels);
          // control words and exchange slots of every matrix in one buffer, armed by one memset
          const size_t ctlBytes = ((size_t)td.ctlStride * scratchBatch * sizeof(unsigned) + 255) / 256 * 256;
          const size_t xchPerMat = (size_t)td.nP * kTile * kTile * sizeof(BT);
          sym.fac.tailCtl.resize(ctlBytes + xchPerMat * scratchBatch);
          sym.fac.tailDinv.resize((size_t)scratchBatch * td.nP * hipk::kDinvSlot * sizeof(BT));
          unsigned* ctl = reinterpret_cast<unsigned*>(sym.fac.tailCtl.ptr) + (size_t)subBatchBase * td.ctlStride;
          BT* xch = reinterpret_cast<BT*>(reinterpret_cast<char*>(sym.fac.tailCtl.ptr) + ctlBytes + xchPerMat * subBatchBase);
          BT* tdinv = const_cast<BT*>(sym.fac.tailDinv.as<BT>()) + (size_t)subBatchBase * td.nP * hipk::kDinvSlot;
          if (subBatchTotal > 0) {  // (a sub-batch arms its own slices only)
            hipCHECK(hipMemsetAsync(ctl, 0xff, (size_t)td.ctlStride * batchSize * sizeof(unsigned), sym.stream));
            hipCHECK(hipMemsetAsync(xch, 0xff, xchPerMat * batchSize, sym.stream));
          } else {
            hipCHECK(hipMemsetAsync(sym.fac.tailCtl.ptr, 0xff, ctlBytes + xchPerMat * scratchBatch, sym.stream));
          }
          timer.begin(kProfChainUpdate);
          hipk::tailFactor<BT><<<dim3((unsigned)hipk::tailRoles(td.nP), gy.y), 256, 0, sym.stream>>>(
              td, ref, tdinv, ctl, xch, sym.asyncErrWord(), (long long)(sym.sweepSpinLimitS * 1e8), sym.tailTrace());
          timer.end();
          sym.counters.tailLaunches++;
        }
        rawValid = false;
        potrfFused = false;
        continue;
      }
      const int slot = dinvSlot;
      dinvSlot ^= 1;
      BT* dinvCur = dinvBase + slot * hipk::kDinvSlot;
      BT* dinvNext = dinvBase + (slot ^ 1) * hipk::kDinvSlot;
      BT* rawCur = rawBase ? rawBase + slot * rawSlot : nullptr;
      BT* rawNext = rawBase ? rawBase + (slot ^ 1) * rawSlot : nullptr;
      const bool fold = nFold > 0 && !potrfFused && plan.foldRank[li] >= 0 && plan.foldRank[li] < nFold;
      if (potrfFused) {
        potrfFused = false;
      } else if (fold) {
        sym.counters.potrfFoldedLevels++;  // (trsmPanelPotrf below; the factors are stored after the last level)
      } else if (nP) {
        timer.begin(kProfPotrf);
        if (direct) {
          hipk::potrfPanelDirect<BT><<<dim3(1, gy.y), 256, 0, sym.stream>>>(
              plan.host.panels[lr.directPanel], ref, dinvCur);
        } else {
          hipk::potrfPanel<BT><<<dim3(nP, gy.y), 256, 0, sym.stream>>>(
              plan.levelPanelDescs.as<PanelDesc>() + lr.panelBegin, ref);
        }
        timer.end();
      }
      // (decided before the trsm launch: with splitK one extra workgroup of that launch already
      //  touches tile 0 of the block-wide segment)
      const bool fuse = direct && lr.directSeg >= 0 && lr.fuseNext && li + 1 < levels.size() &&
                        levels[li + 1].directPanel >= 0 && lr.updEnd > lr.updBegin;
      int splitK = (fuse && nT) ? lr.splitK : 0;
      const bool directUpd = direct && lr.directSeg >= 0 && lr.updEnd > lr.updBegin;
      // does this level's update stage the next panel's rows?
      const bool stage = rawBase && directUpd && lr.rawNext && li + 1 < levels.size() &&
                         levels[li + 1].directPanel >= 0;
      const PanelDesc nextPanel = (stage || fuse) ? plan.host.panels[levels[li + 1].directPanel]
                                                  : PanelDesc{};
      // one launch for trsm + update (+ next potrf): intra-block step whose rows were staged
      // (inside an outer block: K = nb, every source column is solved in the launch; block-last
      //  step: the block-wide source, its leading K - nb columns are final in memory)
      bool merged = false;
      int64_t memOff = 0;
      int kMem = 0;
      if (rawValid && directUpd && nT) {
        const SegDesc& sd = plan.host.segs[lr.directSeg];
        const SrcDesc& sr = plan.host.srcs[sd.src];
        const PanelDesc& pdc = plan.host.panels[lr.directPanel];
        if (!sd.outer && sr.K == pdc.nb) {
          merged = true;
        } else if (sd.outer == 1 && sr.K > pdc.nb && (sr.K - pdc.nb) % kTile == 0 &&
                   sr.rowsBelow == pdc.rowsBelow && sr.lda == pdc.lda) {
          merged = true;
          memOff = sr.off;
          kMem = sr.K - pdc.nb;
        }
      }
      if (merged) splitK = 0;
      bool waitedDef = false;
      if (splitK && lookahead && lr.waitDefLevel >= 0 && defDone[lr.waitDefLevel]) {
        waitDeferred(lr.waitDefLevel);
        waitedDef = true;
      }
      if (nT && !merged) {
        timer.begin(kProfTrsm);
        if (splitK) {
          const SegDesc& sd = plan.host.segs[lr.directSeg];
          SrcDesc part = plan.host.srcs[sd.src];
          part.K = splitK;
          hipk::trsmPanelDirectPlus<BT><<<dim3(nT + 1, gy.y), 256, 0, sym.stream>>>(
              plan.host.panels[lr.directPanel], part, sd, ref, dinvCur);
        } else if (direct) {
          hipk::trsmPanelDirect<BT><<<dim3(nT, gy.y), 256, 0, sym.stream>>>(
              plan.host.panels[lr.directPanel], ref, dinvCur);
        } else if (fold) {
          hipk::trsmPanelPotrf<BT><<<dim3(nT, gy.y), 256, 0, sym.stream>>>(
              plan.trsmTasksFat.as<TrsmTaskFat>() + lr.trsmBegin, ref);
        } else {
          hipk::trsmPanel<BT><<<dim3(nT, gy.y), 256, 0, sym.stream>>>(
              plan.trsmTasksFat.as<TrsmTaskFat>() + lr.trsmBegin, ref);
        }
        timer.end();
      }
      // (a second wait on the same event would still cost a ~6 us bubble between the launches)
      if (!waitedDef && lookahead && lr.waitDefLevel >= 0 && defDone[lr.waitDefLevel]) {
        waitDeferred(lr.waitDefLevel);
      }
      const bool anyDef = lr.defEnd > lr.defBegin;
      auto forkSide = [&]() {
        // (under the source-ordered schedule the fork came AFTER the level's own update launch,
        //  whose "now" tiles ran 3x faster alone than beside freshly started bulk tiles; with the
        //  deadline-ordered units the side stream is busy either way and the earlier fork wins)
        hipEvent_t fork = sym.eventFromPool();
        const hipStream_t side = sym.sideStream();
        hipCHECK(hipEventRecord(fork, sym.stream));
        hipCHECK(hipStreamWaitEvent(side, fork, 0));
        sym.counters.lookaheadForks++;
        // first the tiles the next block's own update must wait for, then (event) the rest:
        // the side stream keeps running them while the chain goes on, and the next block's
        // deferred tiles queue up right behind
        // (one auxiliary stream: the due units simply go ahead of the optional ones on it)
        hipStream_t due = side;
        unsigned dueLds = sym.bulkExtraLds;
        if (dueStream) {
          // due units on their own stream, beside the optional ones (both accumulate with atomics
          // where they can meet: hip_plan.cpp, pushUnit).  They must not overtake the optional
          // units forked two blocks ago, whose far columns are plain read-modify-write.
          due = sym.dueSideStream();
          dueLds = sym.dueExtraLds;
          hipCHECK(hipStreamWaitEvent(due, fork, 0));
          if (lr.flushDue && lastOpt) hipCHECK(hipStreamWaitEvent(due, lastOpt, 0));
          const int64_t f2 = lr.optWaitLevel;
          if (f2 >= 0 && optDone[f2]) hipCHECK(hipStreamWaitEvent(due, optDone[f2], 0));
          dueUsed = true;
        }
        if (lr.defMid > lr.defBegin) {
          timer.begin(kProfUpdate, due);
          launchUpdate(plan, lr.defBegin, lr.defMid, ref, due, nullptr, 0, dueLds, sideMask);
          timer.end();
        }
        defDone[li] = sym.eventFromPool();
        hipCHECK(hipEventRecord(defDone[li], due));
        if (lr.defEnd > lr.defMid) {
          timer.begin(kProfUpdate, side);
          launchUpdate(plan, lr.defMid, lr.defEnd, ref, side, nullptr, 0, sym.bulkExtraLds, sideMask);
          timer.end();
          if (dueStream) {
            optDone[li] = sym.eventFromPool();
            hipCHECK(hipEventRecord(optDone[li], side));
            lastOpt = optDone[li];
          }
        }
        sideUsed = true;
      };
      // (the lookahead units read this level's panel columns and write columns the level's own
      //  update does not touch: they can be forked before it)
      const bool forkEarly = !merged;  // (merged: the panel is solved in the launch)
      if (lookahead && anyDef && forkEarly) forkSide();
      const int64_t updBegin = lr.updBegin;
      if (lr.updEnd > updBegin) {
        timer.begin(direct && lr.directSeg >= 0 ? kProfChainUpdate : kProfUpdate);
        const unsigned nUpd = (unsigned)(lr.updEnd - updBegin);
        if (merged) {
          int kMem0 = kMem, extra = 0;
          if (kMem == 0) {  // intra-block step
            kMem0 = 0;
            if (lr.extraDiag && !extraBroken && fuse) {
              extra = 1;
              extraApplied++;
            } else {
              extraBroken = true;
            }
          } else {          // block-last step: the panels that applied theirs are done
            kMem0 = std::max(0, kMem - kTile * extraApplied);
            extraApplied = 0;
            extraBroken = false;
          }
          hipk::chainStep<BT><<<dim3(nUpd + extra, gy.y), 256, 0, sym.stream>>>(
              plan.host.panels[lr.directPanel], plan.host.segs[lr.directSeg], (int)nUpd, nextPanel,
              fuse ? 1 : 0, ref, rawCur, stage ? rawNext : nullptr, 2 * rawSlot, dinvCur, dinvNext,
              memOff, kMem, (lookahead && batchSize == 1) ? sym.yieldWord() : nullptr,
              sym.traceLaunchId++, kMem0, extra);
          potrfFused = fuse;
        } else if (fuse) {
          if (extraApplied > 0) {
            throw std::runtime_error("HIP backend: internal error (early diagonal updates applied "
                                     "before a step that is not merged)");
          }
          extraBroken = true;
          const SegDesc& sd = plan.host.segs[lr.directSeg];
          hipk::updateTileDirectPotrf<BT><<<dim3(nUpd, gy.y), 256, 0, sym.stream>>>(
              plan.host.srcs[sd.src], sd, (int)nUpd, nextPanel, ref, splitK, dinvNext,
              stage ? rawNext : nullptr, 2 * rawSlot);
          potrfFused = true;
        } else if (direct && lr.directSeg >= 0) {
          if (extraApplied > 0) {
            throw std::runtime_error("HIP backend: internal error (early diagonal updates applied "
                                     "before a step that is not merged)");
          }
          extraBroken = true;
          const SegDesc& sd = plan.host.segs[lr.directSeg];
          hipk::updateTileDirect<BT><<<dim3(nUpd, gy.y), 256, 0, sym.stream>>>(
              plan.host.srcs[sd.src], sd, (int)nUpd, ref, stage ? rawNext : nullptr, nextPanel.nb,
              2 * rawSlot);
        } else {
          auto sp = sym.splitK ? plan.splitRange.find(updBegin) : plan.splitRange.end();
          if (sp != plan.splitRange.end() &&
              (sp->second.second - sp->second.first) * (int64_t)batchSize <= sym.splitKMaxWgs) {
            // (one round of workgroups at most: the K slices of a tile run side by side)
            sym.counters.splitListsUsed++;
            hipk::updateTile<BT, true><<<dim3((unsigned)(sp->second.second - sp->second.first),
                                              (unsigned)batchSize), 256, 0, sym.stream>>>(
                plan.updTasksSplit.as<UpdTaskWide>() + sp->second.first, plan.chainOffTab.as<int64_t>(),
                plan.rowChain.as<int32_t>(), plan.rowLocal.as<int32_t>(), plan.rowColOff.as<int32_t>(), ref,
                nullptr, 0, 1);
          } else {
            launchUpdate(plan, updBegin, lr.updEnd, ref, sym.stream);
          }
        }
        timer.end();
      }
      rawValid = stage;
      if (lookahead && anyDef && !forkEarly) forkSide();
      if (!lookahead) {  // (the same two launches as the lookahead schedule, on the main stream)
        if (lr.defMid > lr.defBegin) {
          timer.begin(kProfUpdate);
          launchUpdate(plan, lr.defBegin, lr.defMid, ref, sym.stream);
          timer.end();
        }
        if (lr.defEnd > lr.defMid) {
          timer.begin(kProfUpdate);
          launchUpdate(plan, lr.defMid, lr.defEnd, ref, sym.stream);
          timer.end();
        }
      }
    }
    if (nFold > 0) {
      // the diagonal blocks of the folded levels: factored (again) and stored, all in one launch --
      // nothing in the factorisation reads them, the solves do
      timer.begin(kProfPotrf);
      hipk::potrfPanel<BT><<<dim3((unsigned)plan.foldPanelEnd[nFold - 1], gy.y), 256, 0, sym.stream>>>(
          plan.foldDescs.as<PanelDesc>(), ref);
      timer.end();
    }
    if (sideUsed) {  // join: everything on the side stream(s) happens-before what follows
      hipEvent_t join = sym.eventFromPool();
      hipCHECK(hipEventRecord(join, sym.sideStream()));
      hipCHECK(hipStreamWaitEvent(sym.stream, join, 0));
    }
    if (dueUsed) {
      hipEvent_t join = sym.eventFromPool();
      hipCHECK(hipEventRecord(join, sym.dueSideStream()));
      hipCHECK(hipStreamWaitEvent(sym.stream, join, 0));
    }
  }

  void launchElim(DevPlan& plan, const ElimRangePlan& er, hipk::DataRef<BT> ref,
                  LaunchTimer& timer) {
    hipk::SkelDev sk = sym.skelDev();
    const unsigned gy = (unsigned)batchSize;
    const int64_t nLumps = er.lumpEnd - er.lumpBegin;
    if (nLumps <= 0) return;
    const unsigned gF = (unsigned)((nLumps + 3) / 4);
    timer.begin(kProfElimFactor);
    if (er.maxWidth <= 4) {
      const int64_t perWg = 4 * hipk::kTinyPerWave;
      hipk::elimFactorTinyStaged<BT><<<dim3((unsigned)((nLumps + perWg - 1) / perWg), gy), 256, 0,
                                      sym.stream>>>(
          plan.elimLumpDesc.as<ElimLumpDesc>() + er.descBegin, ref, (int)nLumps);
    } else if (er.maxWidth <= 8) {
      hipk::elimFactorSmall<BT, 8><<<dim3(gF, gy), 256, 0, sym.stream>>>(sk, ref, er.lumpBegin,
                                                                        er.lumpEnd);
    } else {
      hipk::elimFactorSmall<BT, kElimSmallMax><<<dim3(gF, gy), 256, 0, sym.stream>>>(
          sk, ref, er.lumpBegin, er.lumpEnd);
    }
    timer.end();
    launchLevels(plan, er.bigLevels, ref, timer);
    const int64_t nChains = er.chainEnd - er.chainBegin;
    // FAULT INJECTION (bsp_test_set_fault, tests only): the whole sparse-elimination update is
    // dropped -- the factor of everything the eliminated columns touch is then wrong, and the
    // full-size parity tests must notice (tests/test_full_size_gpu.py)
    if (sym.faultDropElimUpdate) {
      static std::atomic<bool> warned{false};
      if (!warned.exchange(true)) {
        fprintf(stderr, "baspacho_amd: FAULT INJECTION ACTIVE -- sparse-elimination update dropped (tests only)\n");
      }
      return;
    }
    if (er.useGather) {
      const int64_t nItems = er.itemEnd - er.itemBegin;
      if (nItems > 0) {
        timer.begin(kProfElimUpdate);
        hipk::elimGatherMfma<BT><<<dim3((unsigned)((nItems + 3) / 4), gy), 256, 0, sym.stream>>>(
            plan.elimItems.as<ElimGatherItem>() + er.itemBegin, plan.elimPairOffJ.as<uint32_t>(),
            plan.elimPairOffI.as<uint32_t>(), ref, (int)nItems);
        timer.end();
      }
      const int64_t nWide = er.ldsEnd - er.ldsBegin;
      if (nWide > 0) {
        timer.begin(kProfElimUpdate);
        hipk::elimGather<BT><<<dim3((unsigned)((nWide + 3) / 4), gy), 256, 0, sym.stream>>>(
            plan.elimItems.as<ElimGatherItem>() + er.ldsBegin, plan.elimPairOffJ.as<uint32_t>(),
            plan.elimPairOffI.as<uint32_t>(), ref, (int)nWide);
        timer.end();
      }
      const int64_t nTiny9 = er.tiny9End - er.tinyBegin, nTiny = er.tinyEnd - er.tiny9End;
      if (nTiny9 > 0) {  // 7 items per wave, 28 per workgroup
        timer.begin(kProfElimUpdate);
        hipk::elimGatherTiny<BT, 9><<<dim3((unsigned)((nTiny9 + 27) / 28), gy), 256, 0, sym.stream>>>(
            plan.elimItems.as<ElimGatherItem>() + er.tinyBegin, plan.elimPairOffJ.as<uint32_t>(),
            plan.elimPairOffI.as<uint32_t>(), ref, (int)nTiny9);
        timer.end();
      }
      if (nTiny > 0) {
        timer.begin(kProfElimUpdate);
        hipk::elimGatherTiny<BT, 16><<<dim3((unsigned)((nTiny + 15) / 16), gy), 256, 0, sym.stream>>>(
            plan.elimItems.as<ElimGatherItem>() + er.tiny9End, plan.elimPairOffJ.as<uint32_t>(),
            plan.elimPairOffI.as<uint32_t>(), ref, (int)nTiny);
        timer.end();
      }
    } else if (nChains > 0) {
      timer.begin(kProfElimUpdate);
      hipk::elimUpdate<BT><<<dim3((unsigned)((nChains + 3) / 4), gy), 256, 0, sym.stream>>>(
          sk, plan.elimChainLump.as<int32_t>() + er.chainLumpOff, ref, er.chainBegin, er.chainEnd);
      timer.end();
    }
  }

  virtual bool hasFusedFactor() const override { return !sym.forcePerOp; }

  // every launch of a factor over `plan`, in order, on sym.stream and the auxiliary streams
  void enqueueFactor(DevPlan& plan, hipk::DataRef<BT> ref, LaunchTimer& timer) {
    sym.resetEventPool();
    // CONCURRENT SUB-BATCHES (round 5).  A large batch of a latency-bound structure is three dependent
    // launches per tree level, each with a ramp and a tail in which most of the GPU idles; two halves
    // of the batch on two streams fill each other's (64 x GRID 82x82: 10.76 -> 10.2 ms with two Solver
    // clones on two streams, profiles/r3_concurrent_batch.py re-run in round 5; four halves: host
    // enqueue bound, slower).  The second half runs on the auxiliary stream, which such a plan does
    // not use for lookahead; matrices are independent, the halves share nothing but the plan.
    const bool lookahead = lookaheadOn() && plan.host.lookaheadPays(batchSize, sym.lookaheadMinFlops);
    if (ref.many && !lookahead && sym.profile == nullptr && batchSize >= sym.subBatchMin) {
      const int total = batchSize;
      const int parts = std::max(2, std::min({sym.subBatchParts, 4, total / std::max(1, sym.subBatchMin / 2)}));
      hipStream_t mainStream = sym.stream;
      hipEvent_t fork = sym.eventFromPool();
      hipCHECK(hipEventRecord(fork, mainStream));  // (the pointer array has been copied on this stream)
      struct Restore {
        HipNumericCtx& c;
        hipStream_t st;
        int bs;
        ~Restore() {
          c.sym.stream = st;
          c.batchSize = bs;
          c.subBatchBase = c.subBatchTotal = 0;
        }
      } restore{*this, mainStream, total};
      subBatchTotal = total;
      for (int g = 0; g < parts; g++) {
        const int b0 = (int)((int64_t)total * g / parts), b1 = (int)((int64_t)total * (g + 1) / parts);
        subBatchBase = b0;
        batchSize = b1 - b0;
        sym.stream = g ? sym.streams().batch[g - 1] : mainStream;
        if (g) hipCHECK(hipStreamWaitEvent(sym.stream, fork, 0));
        sym.counters.subBatchesEnqueued++;
        hipk::DataRef<BT> sub{nullptr, ref.many + subBatchBase};
        for (const ElimRangePlan& er : plan.host.elimRanges) launchElim(plan, er, sub, timer);
        launchLevels(plan, plan.host.levels, sub, timer);
        if (g) {
          hipEvent_t join = sym.eventFromPool();
          hipCHECK(hipEventRecord(join, sym.stream));
          hipCHECK(hipStreamWaitEvent(mainStream, join, 0));
        }
      }
      return;
    }
    for (const ElimRangePlan& er : plan.host.elimRanges) launchElim(plan, er, ref, timer);
    launchLevels(plan, plan.host.levels, ref, timer);
  }

  // (factor() as ONE captured hipGraph launch was built in round 2 and measured no faster on this
  //  stack -- GRID 82x82 1.66-1.79 against 1.74-1.77 ms, BAL-871 7.15 = 7.16: the runtime plays a
  //  graph back as the same packets on the same queues -- and removed in round 4)
  virtual void factorRange(T* data, int64_t startLump, int64_t upToLump) override {
    sym.checkAsyncError();
    DevPlan* planPtr = &sym.planFor(sym.sparseElimRanges, startLump, upToLump, /*tag=*/0);
    if (batchSize > 1 && planPtr->host.hasTail) {
      planPtr = &sym.planFor(sym.sparseElimRanges, startLump, upToLump, /*tag=*/2);
    }
    DevPlan& plan = *planPtr;
    hipk::DataRef<BT> ref = makeRef(data);
    LaunchTimer timer(sym.stream, sym.profile);
    enqueueFactor(plan, ref, timer);
    hipCHECK(hipGetLastError());
    timer.finish();
  }

  // host array of the matrices' device pointers (one entry for a single matrix)
  void dataPointers(T* data, vector<BT*>& out);

  virtual void doElimination(const SymElimCtx& elimData, T* data, int64_t lumpsBegin,
                             int64_t lumpsEnd) override {
    const HipSymElimCtx* e = dynamic_cast<const HipSymElimCtx*>(&elimData);
    BASPACHO_CHECK_NOTNULL(e);
    BASPACHO_CHECK_EQ(e->lumpsBegin, lumpsBegin);
    BASPACHO_CHECK_EQ(e->lumpsEnd, lumpsEnd);
    DevPlan& plan = sym.planFor({lumpsBegin, lumpsEnd}, lumpsBegin, lumpsEnd, /*tag=*/1);
    hipk::DataRef<BT> ref = makeRef(data);
    LaunchTimer timer(sym.stream, sym.profile);
    sym.resetEventPool();
    for (const ElimRangePlan& er : plan.host.elimRanges) launchElim(plan, er, ref, timer);
    hipCHECK(hipGetLastError());
    timer.finish();
  }

  // ---- per-op boundary (MatOps.h:113-136).  factor() never goes through these (fused path); they
  // exist so that a driver written against the reference's NumericCtx -- e.g. the per-op loop of
  // Solver.cpp:198-218, kept in solver.cpp -- runs on this backend op by op.  Each call builds a
  // one-off device plan: correct, not fast.
  DevPlan& adoptPlan(HipPlanHost&& host) {
    opPlans.emplace_back(new DevPlan);
    opPlans.back()->host = std::move(host);
    opPlans.back()->upload();
    return *opPlans.back();
  }

  virtual void potrf(int64_t n, T* data, int64_t offA) override {
    sym.potrfBiggestN = std::max(sym.potrfBiggestN, n);
    DevPlan& plan = adoptPlan(buildDenseOpPlan(n, 0, offA, /*potrfOnly=*/true));
    OpTimer opTimer(sym.potrfStat, sym.stream, (double)n);
    LaunchTimer timer(sym.stream, nullptr);
    {
      FlagOff noLookahead(sym.lookaheadEnabled);
      launchLevels(plan, plan.host.levels, makeRef(data), timer);
    }
    hipCHECK(hipGetLastError());
  }

  virtual void trsm(int64_t n, int64_t k, T* data, int64_t offA, int64_t offB) override {
    // every caller on the factor path passes the rows that directly follow the diagonal block
    // (Solver.cpp:43-64); the blocked solve relies on that contiguity
    BASPACHO_CHECK_EQ(offB, offA + n * n);
    DevPlan& plan = adoptPlan(buildDenseOpPlan(n, k, offA, /*potrfOnly=*/false));
    OpTimer opTimer(sym.trsmStat, sym.stream, (double)n, (double)k);
    LaunchTimer timer(sym.stream, nullptr);
    {
      FlagOff noLookahead(sym.lookaheadEnabled);
      launchLevels(plan, plan.host.levels, makeRef(data), timer);
    }
    hipCHECK(hipGetLastError());
  }

  virtual void saveSyrkGemm(int64_t m, int64_t n, int64_t k, const T* data, int64_t offset) override {
    BASPACHO_CHECK_LE(m * n, tempBufSize);
    temp.resize((size_t)(tempBufSize * batchSize) * sizeof(BT));
    hipCHECK(hipMemsetAsync(temp.ptr, 0, (size_t)(tempBufSize * batchSize) * sizeof(BT), sym.stream));
    HipPlanHost host;
    SrcDesc sr{};
    sr.off = offset;
    sr.lda = (int32_t)k;
    sr.K = (int32_t)k;
    sr.rowsBelow = (int32_t)n;
    sr.nRest = (int32_t)n;
    host.srcs.push_back(sr);
    SegDesc sd{};
    sd.src = 0;
    sd.kind = kSegIntra;
    sd.q0 = 0;
    sd.m = (int32_t)m;
    sd.tgtBase = 0;
    sd.tgtStride = (int32_t)m;
    host.segs.push_back(sd);
    for (int32_t cT = 0; cT < m; cT += kTile) {
      for (int32_t rT = cT; rT < n; rT += kTile) host.updTasks.push_back({0, rT, cT, 0});
    }
    DevPlan& plan = adoptPlan(std::move(host));
    sym.gemmCalls++;
    OpTimer opTimer(sym.sygeStat, sym.stream, (double)m, (double)n, (double)k);
    // temp := -(P P^T) on the lower trapezoid (the strictly upper part of the leading m x m block
    // "doesn't matter", MatOps.h:129); assemble() adds it
    launchUpdate(plan, 0, plan.numUpdTasks, makeRef(const_cast<T*>(data)),
                 sym.stream, temp.as<BT>() ? const_cast<BT*>(temp.as<BT>()) : nullptr, tempBufSize);
    hipCHECK(hipGetLastError());
  }

  virtual void prepareAssemble(int64_t targetLump) override {
    hipk::SkelDev sk = sym.skelDev();
    spanToChainOffset.resize((size_t)(sym.skel.numSpans() + 1) * sizeof(int64_t));
    const int64_t n = sym.skel.chainColPtr[targetLump + 1] - sym.skel.chainColPtr[targetLump];
    hipk::prepareAssembleKernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, sym.stream>>>(
        sk, reinterpret_cast<int64_t*>(spanToChainOffset.ptr), targetLump);
  }

  virtual void assemble(T* data, int64_t rectRowBegin, int64_t dstStride, int64_t srcColDataOffset,
                        int64_t srcRectWidth, int64_t numBlockRows, int64_t numBlockCols) override {
    hipk::SkelDev sk = sym.skelDev();
    OpTimer opTimer(sym.asmblStat, sym.stream, (double)numBlockRows, (double)numBlockCols);
    hipk::assembleKernel<BT><<<dim3((unsigned)numBlockRows, (unsigned)batchSize), 256, 0, sym.stream>>>(
        sk, spanToChainOffset.as<int64_t>(), temp.as<BT>(), tempBufSize, makeRef(data),
        rectRowBegin, dstStride, srcColDataOffset, srcRectWidth, numBlockRows, numBlockCols);
    hipCHECK(hipGetLastError());
  }

  virtual void pseudoFactorSpans(T* data, int64_t spanBegin, int64_t spanEnd) override {
    if (spanEnd <= spanBegin) return;
    const CoalescedBlockMatrixSkel& sk = sym.skel;
    // spans of up to kElimSmallMax columns: one wave per span (diagonal block in LDS, rows in
    // registers).  Wider spans (the reference has no width limit, MatOpsCuda.cu:188-233) go through
    // the panel potrf / trsm kernels, one dense-op plan per span; runs of narrow spans in between
    // are batched into one launch each.
    hipk::DataRef<BT> ref = makeRef(data);
    auto narrowRun = [&](int64_t b, int64_t e) {
      if (e <= b) return;
      hipk::pseudoFactorSpansKernel<BT><<<dim3((unsigned)((e - b + 3) / 4), (unsigned)batchSize), 256,
                                          0, sym.stream>>>(sym.skelDev(), ref, b, e);
    };
    FlagOff noLookahead(sym.lookaheadEnabled);
    int64_t runBegin = spanBegin;
    for (int64_t s = spanBegin; s < spanEnd; s++) {
      const int64_t n = sk.spanStart[s + 1] - sk.spanStart[s];
      if (n <= kElimSmallMax) continue;
      narrowRun(runBegin, s);
      runBegin = s + 1;
      const int64_t lump = sk.spanToLump[s];
      const int64_t lda = sk.lumpStart[lump + 1] - sk.lumpStart[lump];
      const int64_t c0 = sk.chainColPtr[lump], nCh = sk.chainColPtr[lump + 1] - c0;
      const int64_t idxInLump = s - sk.lumpToSpan[lump];
      // (the chains of a lump column follow each other: the rows below the span's diagonal block
      //  start n rows after it)
      const int64_t offD = sk.chainData[c0 + idxInLump] + sk.spanOffsetInLump[s];
      const int64_t rowsBelow = sk.chainRowsTillEnd[c0 + nCh - 1] - sk.chainRowsTillEnd[c0 + idxInLump];
      LaunchTimer timer(sym.stream, nullptr);
      DevPlan& pf = adoptPlan(buildDenseOpPlan(n, 0, offD, /*potrfOnly=*/true, 0, lda));
      launchLevels(pf, pf.host.levels, ref, timer);
      if (rowsBelow > 0) {
        DevPlan& ps = adoptPlan(buildDenseOpPlan(n, rowsBelow, offD, /*potrfOnly=*/false, 0, lda));
        launchLevels(ps, ps.host.levels, ref, timer);
      }
    }
    narrowRun(runBegin, spanEnd);
    hipCHECK(hipGetLastError());
  }

  HipSymbolicCtx& sym;
  int batchSize;
  int subBatchBase = 0, subBatchTotal = 0;  // enqueueFactor: the sub-batch being enqueued
  int64_t tempBufSize = 0;
  DevBuf temp, spanToChainOffset;  // per-op boundary only (saveSyrkGemm / prepareAssemble)
  vector<std::unique_ptr<DevPlan>> opPlans;
};

template <>
hipk::DataRef<double> HipNumericCtx<double>::makeRef(double* data) {
  return {data, nullptr};
}
template <>
hipk::DataRef<float> HipNumericCtx<float>::makeRef(float* data) {
  return {data, nullptr};
}
template <>
void HipNumericCtx<double>::dataPointers(double* data, vector<double*>& out) { out = {data}; }
template <>
void HipNumericCtx<float>::dataPointers(float* data, vector<float*>& out) { out = {data}; }
template <>
void HipNumericCtx<vector<double*>>::dataPointers(vector<double*>* data, vector<double*>& out) {
  BASPACHO_CHECK_EQ((int)data->size(), batchSize);
  out = *data;
}
template <>
void HipNumericCtx<vector<float*>>::dataPointers(vector<float*>* data, vector<float*>& out) {
  BASPACHO_CHECK_EQ((int)data->size(), batchSize);
  out = *data;
}
template <>
hipk::DataRef<double> HipNumericCtx<vector<double*>>::makeRef(vector<double*>* data) {
  BASPACHO_CHECK_EQ((int)data->size(), batchSize);
  return {nullptr, (double* const*)sym.fac.ptrRing.push(data->data(), data->size() * sizeof(double*),
                                                    sym.stream)};
}
template <>
hipk::DataRef<float> HipNumericCtx<vector<float*>>::makeRef(vector<float*>* data) {
  BASPACHO_CHECK_EQ((int)data->size(), batchSize);
  return {nullptr, (float* const*)sym.fac.ptrRing.push(data->data(), data->size() * sizeof(float*),
                                                   sym.stream)};
}

}  // namespace

NumericCtxBase* hipb::createHipNumericCtx(HipSymbolicCtx& sym, std::type_index tIdx, int64_t tempSize, int batch) {
  if (tIdx == std::type_index(typeid(double))) return new HipNumericCtx<double>(sym, 1, tempSize);
  if (tIdx == std::type_index(typeid(float))) return new HipNumericCtx<float>(sym, 1, tempSize);
  if (tIdx == std::type_index(typeid(vector<double*>))) {
    return new HipNumericCtx<vector<double*>>(sym, batch, tempSize);
  }
  if (tIdx == std::type_index(typeid(vector<float*>))) {
    return new HipNumericCtx<vector<float*>>(sym, batch, tempSize);
  }
  return nullptr;
}

void hipb::launchFactorWarmup(hipStream_t stream) { hipk::warmupKernel<<<1, 64, 0, stream>>>(); }

int hipBackendReadExtents(unsigned long long* out, int maxLaunches) {
#if defined(BSP_KTRACE) && defined(BSP_TRACE_TILE)
  hipCHECK(hipDeviceSynchronize());
  const int n = std::min(maxLaunches, 2048);
  hipCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(hipk::bspLaunchExtent), sizeof(unsigned long long) * 4 * n));
  // reset: minima to the largest value, maxima to zero
  std::vector<unsigned long long> init(2048 * 4, 0ull);
  for (int i = 0; i < 2048; i++) init[4 * i] = ~0ull;
  hipCHECK(hipMemcpyToSymbol(HIP_SYMBOL(hipk::bspLaunchExtent), init.data(), sizeof(unsigned long long) * 4 * 2048));
  return n;
#else
  (void)out;
  (void)maxLaunches;
  return 0;
#endif
}

int hipBackendReadTrace(long long* out, int maxRecords) {
#if defined(BSP_KTRACE) || defined(BSP_TRACE_UPD)
  unsigned n = 0;
  hipCHECK(hipDeviceSynchronize());
  hipCHECK(hipMemcpyFromSymbol(&n, HIP_SYMBOL(hipk::bspTraceCount), sizeof n));
  const int cnt = (int)std::min<unsigned>(n, (unsigned)std::min(maxRecords, 8192));
  hipCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(hipk::bspTrace), sizeof(long long) * hipk::kTraceW * cnt));
  n = 0;
  hipCHECK(hipMemcpyToSymbol(HIP_SYMBOL(hipk::bspTraceCount), &n, sizeof n));
  return cnt;
#else
  (void)out;
  (void)maxRecords;
  return 0;
#endif
}

double hipBackendMfmaF64ProbeTflops() {
  const int blocks = 1024, iters = 4000;
  double* out = nullptr;
  hipCHECK(hipMalloc(&out, sizeof(double) * 256 * blocks));
  hipEvent_t a, b;
  hipCHECK(hipEventCreate(&a));
  hipCHECK(hipEventCreate(&b));
  hipk::mfmaF64Probe<<<blocks, 256>>>(out, iters);  // warm-up
  hipCHECK(hipEventRecord(a, nullptr));
  hipk::mfmaF64Probe<<<blocks, 256>>>(out, iters);
  hipCHECK(hipEventRecord(b, nullptr));
  hipCHECK(hipEventSynchronize(b));
  float ms = 0;
  hipCHECK(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  (void)hipFree(out);
  return double(blocks) * 4 * iters * 4 * 2048.0 / (ms * 1e-3) / 1e12;
}

}  // namespace BaSpaCho
