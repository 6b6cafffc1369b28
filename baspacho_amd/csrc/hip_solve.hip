// MI355X backend, the solve launch path: triangular solves on the device, fused over a lump range
// (SolveCtx extension of mat_ops.h), with the kernels of hip_solve_kernels.h, hip_solve_wide.h and
// the persistent sweeps of hip_sweep_kernels.h / hip_sweep_mfma.h.
#include "hip_context.h"
#include "hip_solve_kernels.h"
#include "hip_solve_wide.h"
#include "hip_sweep_kernels.h"
#include "hip_sweep_mfma.h"

namespace BaSpaCho {

using std::vector;
using namespace hipb;

namespace {

// Triangular solves on the device, fused over a lump range (SolveCtx extension of mat_ops.h).
template <typename T>
struct HipSolveCtx : SolveCtx<T> {
  using BT = BaseType<T>;
  HipSolveCtx(HipSymbolicCtx& sym_, int nRHS_, int batch_) : sym(sym_), nRHS(nRHS_), batch(batch_) {}

  // (TESTING switch hipBackendForcePerOp: the solver then drives the reference's op-by-op loops,
  //  Solver.cpp:303-328,357-381,419-448, over the per-op virtuals below)
  virtual bool hasFusedSolve() const override { return !sym.forcePerOp; }

  dim3 grid(unsigned x) const { return dim3(x, (unsigned)nRHS, (unsigned)batch); }

  template <bool BACKWARD>
  void elimRange(DevPlan& plan, const ElimRangePlan& er, hipk::SolveRef<BT> ref) {
    hipk::SkelDev sk = sym.skelDev();
    const int64_t nLumps = er.lumpEnd - er.lumpBegin;
    if (nLumps <= 0) return;
    auto small = [&] {
      const dim3 gL = grid((unsigned)((nLumps + 255) / 256));
      plan.ensureSolveGather(sym.skel);
      if (BACKWARD) {
        if (er.maxWidth <= 4) {
          const int64_t d0 = plan.solveGather.rangeLumpDesc[&er - plan.host.elimRanges.data()];
          // (several right-hand sides per workgroup: the blocks of L are fetched once per group)
          auto launch = [&](auto kern, int rb) {
            kern<<<dim3((unsigned)((nLumps + 15) / 16), (unsigned)((nRHS + rb - 1) / rb), (unsigned)batch),
                   256, 0, sym.stream>>>(plan.solveLumpDescs.as<SolveLumpDesc>() + d0,
                                         plan.solveLumpBlocks.as<SolveLumpBlock>(), ref, (int)nLumps, nRHS);
          };
          const auto wide = plan.solveGather.rangeWide[&er - plan.host.elimRanges.data()];
          const int64_t wideRows = sym.skel.order() - wide.rowBelow;
          const int64_t wideSpans = (int64_t)sym.skel.spanStart.size() - 1 - wide.spanBelow;
          const unsigned wideGroups = (unsigned)((nRHS + hipk::kWideRhs - 1) / hipk::kWideRhs);
          const size_t wideBytes = (size_t)hipk::wideGroupStride(wideRows) * wideGroups * (size_t)batch * sizeof(BT);
          if (nRHS == 1) {
            hipk::solveElimLumpsLt<BT><<<grid((unsigned)((nLumps + 15) / 16)), 256, 0, sym.stream>>>(
                plan.solveLumpDescs.as<SolveLumpDesc>() + d0, plan.solveLumpBlocks.as<SolveLumpBlock>(),
                ref, (int)nLumps);
          } else if (sym.solveWide && wide.n >= 1 && nRHS >= sym.solveWideMinRhs &&
                     wideBytes <= sym.solveWideMaxBytes) {
            // right-hand sides across the lanes (hip_solve_wide.h): the rows below the range, final by
            // now, go span by span into [16][rows] blocks first
            sym.sol.solveWideBuf.resize(wideBytes);
            BT* yW = const_cast<BT*>(sym.sol.solveWideBuf.as<BT>());
            if (wideSpans > 0) {
              hipk::solveRowsToWide<BT><<<dim3((unsigned)((wideSpans + 3) / 4), wideGroups, (unsigned)batch),
                                          256, 0, sym.stream>>>(ref, nRHS, sk.spanStart, wide.spanBelow,
                                                                wideSpans, wide.rowBelow, wideRows, yW);
            }
            auto launchW = [&](auto kern) {
              kern<<<dim3((unsigned)((nLumps + 15) / 16), wideGroups, (unsigned)batch), 256, 0, sym.stream>>>(
                  plan.solveLumpDescs.as<SolveLumpDesc>() + d0, plan.solveLumpBlocks.as<SolveLumpBlock>(),
                  ref, (int)nLumps, nRHS, yW, wide.rowBelow, wideRows);
            };
            switch (wide.n) {
              case 1: launchW(hipk::solveElimLumpsLtWide<BT, 1>); break;
              case 2: launchW(hipk::solveElimLumpsLtWide<BT, 2>); break;
              case 3: launchW(hipk::solveElimLumpsLtWide<BT, 3>); break;
              default: launchW(hipk::solveElimLumpsLtWide<BT, 4>); break;
            }
            sym.counters.solveWideLaunches++;
          } else if (nRHS <= 2) {
            launch(hipk::solveElimLumpsLtMulti<BT, 2>, 2);
          } else if (nRHS <= 4) {
            launch(hipk::solveElimLumpsLtMulti<BT, 4>, 4);
          } else {
            launch(hipk::solveElimLumpsLtMulti<BT, 8>, 8);
          }
        } else {
          hipk::solveElimSmall<BT, true><<<gL, 256, 0, sym.stream>>>(sk, ref, er.lumpBegin,
                                                                    er.lumpEnd);
        }
        return;
      }
      const auto items = plan.solveGather.rangeItems[&er - plan.host.elimRanges.data()];
      // (every right-hand side in the thread / 16 right-hand sides per workgroup: L is read once)
      hipk::solveElimDiagL<BT><<<dim3((unsigned)((nLumps + 255) / 256), 1, (unsigned)batch), 256, 0,
                                 sym.stream>>>(sk, ref, er.lumpBegin, er.lumpEnd, nRHS);
      if (items.second > items.first) {
        hipk::solveElimGatherL<BT><<<dim3((unsigned)(items.second - items.first),
                                          (unsigned)((nRHS + 15) / 16), (unsigned)batch),
                                     256, 0, sym.stream>>>(
            plan.solveItems.as<SolveGatherItem>() + items.first,
            plan.solveEntries.as<SolveGatherEntry>(), ref, nRHS);
      }
    };
    // lumps of a range are mutually independent: the order small/wide does not matter
    if (!BACKWARD) {
      small();
      denseLevels<false>(plan, er.bigLevels, ref);
    } else {
      denseLevels<true>(plan, er.bigLevels, ref);
      small();
    }
  }

  // The steps of a level list (buildSolveSchedule, hip_plan.h), and the upload of the panels whose
  // diagonal blocks are inverted
  void buildSchedule(DevPlan& plan, const vector<LevelRange>& levels, bool withSweeps,
                     SolveInvList& ent) {
    static_assert(hipk::kSolveBlock == kOuterWidth, "block solve steps = outer blocks of the plan");
    static_cast<SolveSchedule&>(ent) = buildSolveSchedule(
        plan.host, levels, {withSweeps, sym.blockSolve, sym.solveInv && sym.blockSolve, sym.sweepMinWidth});
    ent.count = (int64_t)ent.invPanels.size();
    if (ent.count) ent.list.upload(ent.invPanels);
    ent.built = true;
  }

  // may this call run the sweeps of `ent`?  Every workgroup of a sweep launch should be resident at
  // once (correct either way -- roles are dealt by ticket -- but a far role that starts late has a
  // whole row strip to catch up on at one CU's bandwidth), and its LDS must fit.
  // (several right-hand sides: the matrix-core sweep, 16 right-hand sides per set of workgroups)
  // (the matrix-core sweep pays on LONG runs only: a step is 16-17 us whatever the width below it, the block
  //  path's two launches per 256 columns cost less while the rows below are few; profiles/r06_solve10_families.txt)
  bool sweepMfma(const SolveInvList& ent) const {
    return nRHS >= sym.sweepMfmaMinRhs && ent.maxSweepW >= sym.sweepMfmaMinWidth;
  }
  // may the persistent sweeps be launched here?  (attributes of the four kernels, the watchdog word)
  bool sweepReady() {
    int& st = sym.sol.sweepAttr[sizeof(BT) == 8 ? 0 : 1];
    if (st == 0) {
      st = -1;
      sym.checkDevice();
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, sym.device) == hipSuccess) {
        sym.sol.sweepCapacity = prop.multiProcessorCount;
        sym.sol.sweepMaxLds = std::min<size_t>(prop.maxSharedMemoryPerMultiProcessor, 160 * 1024) - 1024;
        const int lds = (int)sym.sol.sweepMaxLds;
        bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&hipk::solveSweep<BT, false>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
        ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(&hipk::solveSweep<BT, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
        ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(&hipk::solveSweepM<BT, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
        ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(&hipk::solveSweepM<BT, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
        ok = ok && sym.allocAsyncErrWord() == hipSuccess;
        if (ok) st = 1;
      }
      if (st < 0) (void)hipGetLastError();
    }
    return st > 0;
  }
  bool sweepsFit(const SolveInvList& ent) {
    if (ent.numSweeps == 0) return false;
    if (!sweepReady()) return false;
    if (sweepMfma(ent)) {
      const int64_t inst = (int64_t)((nRHS + hipk::kSweepR - 1) / hipk::kSweepR) * batch;
      return ent.maxSweepWgsM * inst <= sym.sol.sweepCapacity && hipk::sweepMLdsBytes<BT>() <= sym.sol.sweepMaxLds;
    }
    const int64_t inst = (int64_t)nRHS * batch;
    if (ent.maxSweepWgs * inst > sym.sol.sweepCapacity) return false;
    const size_t lds = std::max(hipk::sweepLdsBytes<BT>(ent.maxSweepW, ent.maxSweepBelow, false),
                                hipk::sweepLdsBytes<BT>(ent.maxSweepW, ent.maxSweepBelow, true));
    return lds <= sym.sol.sweepMaxLds;
  }

  template <bool BACKWARD>
  void denseLevels(DevPlan& plan, const vector<LevelRange>& levels, hipk::SolveRef<BT> ref) {
    // schedule: with persistent sweeps when the plan has wide runs and this call fits the GPU
    SolveInvList* entp = nullptr;
    if (sym.sweepUsable()) {
      SolveInvList& es = plan.solveInvLists[{&levels, 1}];
      if (!es.built) buildSchedule(plan, levels, true, es);
      if (sweepsFit(es)) entp = &es;
    }
    if (!entp) {
      SolveInvList& eo = plan.solveInvLists[{&levels, 0}];
      if (!eo.built) buildSchedule(plan, levels, false, eo);
      entp = &eo;
    }
    SolveInvList& ent = *entp;
    const bool sweeps = ent.numSweeps > 0 && entp == &plan.solveInvLists[{&levels, 1}];
    const int64_t nG = (int64_t)ent.items.size();
    // round 3 (BSP_SOLVE_INV=0 disables): the block triangles through inverted 64 x 64 diagonal
    // blocks -- one launch inverts the diagonal block of every panel of every block group and sweep
    // (the list of those panels is built and uploaded once per level list), the block kernel then
    // needs one round trip (hip_solve_kernels.h, K-B0 / K-B1i).  Round 6: the same launch arms the
    // exchange buffer of the sweeps.
    const BT* invBase = nullptr;
    int64_t invBatchStride = 0;
    BT* xchg = nullptr;
    hipk::SweepShared sh{};
    const bool mfma = sweeps && sweepMfma(ent);
    const int64_t rhsGroups = mfma ? (nRHS + hipk::kSweepR - 1) / hipk::kSweepR : nRHS;
    const int64_t nInst = rhsGroups * batch;
    const int64_t instStride = ent.sweepInstStride * (mfma ? hipk::kSweepR : 1);
    if (ent.count > 0) {
      invBatchStride = ent.count * kPanelWidth * kPanelWidth;
      sym.sol.solveInvScratch.resize((size_t)(invBatchStride * batch) * sizeof(BT));
      BT* scratch = const_cast<BT*>(sym.sol.solveInvScratch.as<BT>());
      unsigned long long* arm = nullptr;
      int64_t armWords = 0;
      if (sweeps) {
        const size_t ctlBytes = (((size_t)(1 + ent.numSweeps * nInst) * sizeof(unsigned)) + 255) / 256 * 256;
        const size_t bytes = (ctlBytes + (size_t)(nInst * instStride) * sizeof(BT) + 7) / 8 * 8;
        sym.sol.sweepXchg.resize(bytes);
        arm = reinterpret_cast<unsigned long long*>(sym.sol.sweepXchg.ptr);
        armWords = (int64_t)(bytes / 8);
        xchg = reinterpret_cast<BT*>(reinterpret_cast<char*>(sym.sol.sweepXchg.ptr) + ctlBytes);
        sh.ctl = reinterpret_cast<unsigned*>(sym.sol.sweepXchg.ptr);
        sh.hostErr = sym.sol.errWord.dev;
        sh.spinLimit = (long long)(sym.sweepSpinLimitS * 1e8);
        sh.instStride = instStride;
        sh.fault = sym.sweepFault;
        sh.pad = 0;
        sh.trace = nullptr;
        if (sym.sweepTraceOn) {
          sym.sol.sweepTrace.resize(8 * 4096 * sizeof(long long));
          sh.trace = reinterpret_cast<long long*>(sym.sol.sweepTrace.ptr);
        }
      }
      // (solve() = solveL then solveLt through ONE context, on the same factor: the backward pass finds
      //  the inverses its forward pass left in the scratch -- nothing else has written it in between --
      //  and only arms the exchange buffer)
      if (invCacheList == &ent && invCacheGen == sym.solveInvGen && invCacheGen != 0) {
        if (arm) hipCHECK(hipMemsetAsync(arm, 0xff, (size_t)armWords * 8, sym.stream));
        sym.counters.invReused++;
      } else {
        hipk::solveInvertPanels<BT><<<dim3((unsigned)ent.count, 1, (unsigned)batch), 64, 0, sym.stream>>>(
            ent.list.as<PanelDesc>(), scratch, invBatchStride, ref, arm, armWords);
        invCacheList = &ent;
        invCacheGen = ++sym.solveInvGen;
      }
      invBase = scratch;
    }
    int32_t sweepOrd = 0;
    for (int64_t gi = 0; gi < nG; gi++) {
      const int64_t gIdx = BACKWARD ? nG - 1 - gi : gi;
      const SolveSchedItem& item = ent.items[gIdx];
      if (item.kind == SolveSchedItem::kSweep) {
        hipk::SweepDesc sd = item.sweep;
        sd.ticketOff = (int32_t)((BACKWARD ? ent.numSweeps - 1 - sweepOrd : sweepOrd) * nInst);
        sweepOrd++;
        if (mfma) {
          const unsigned gx = (unsigned)(BACKWARD ? hipk::kSweepFwdGroup * sd.nBlocks : item.sweepFwdWgs);
          hipk::solveSweepM<BT, BACKWARD><<<dim3(gx, (unsigned)rhsGroups, (unsigned)batch), 256,
                                           hipk::sweepMLdsBytes<BT>(), sym.stream>>>(
              sd, nRHS, invBase, invBatchStride, xchg, sh, plan.rowGlobal.as<int32_t>(), ref);
          sym.counters.sweepLaunches++;
          sym.counters.sweepMfmaLaunches++;
          continue;
        }
        const size_t lds = hipk::sweepLdsBytes<BT>(sd.w, sd.rowsBelow, BACKWARD);
        const unsigned gx = (unsigned)(BACKWARD ? item.sweepBwdWgs : item.sweepFwdWgs);
        hipk::solveSweep<BT, BACKWARD><<<grid(gx), 256, lds, sym.stream>>>(
            sd, invBase, invBatchStride, xchg, sh, plan.rowGlobal.as<int32_t>(), ref);
        sym.counters.sweepLaunches++;
        continue;
      }
      if (item.kind == SolveSchedItem::kBlockGroup) {
        const PanelDesc& first = plan.host.panels[levels[item.l].directPanel];
        const PanelDesc& last = plan.host.panels[levels[item.e - 1].directPanel];
        const int w = (int)(item.e - 1 - item.l) * kPanelWidth + last.nb;
        const unsigned nT = (unsigned)((last.rowsBelow + kTile - 1) / kTile);
        if (invBase && item.slot >= 0) {
          const BT* inv = invBase + (int64_t)item.slot * kPanelWidth * kPanelWidth;
          if (!BACKWARD) {
            hipk::solveTriBlockInv<BT, false><<<grid(1), 256, 0, sym.stream>>>(first, w, inv, invBatchStride, ref);
            if (nT) {
              hipk::solveGemvBlockL<BT><<<grid(nT), 256, 0, sym.stream>>>(
                  first, last, w, plan.rowGlobal.as<int32_t>(), ref);
            }
          } else {
            if (nT) {
              hipk::solveGemvBlockLt<BT><<<grid(nT), 256, 0, sym.stream>>>(
                  first, last, w, plan.rowGlobal.as<int32_t>(), ref);
            }
            hipk::solveTriBlockInv<BT, true><<<grid(1), 256, 0, sym.stream>>>(first, w, inv, invBatchStride, ref);
          }
          continue;
        }
        if (!BACKWARD) {
          hipk::solveTriBlock<BT, false><<<grid(1), 256, 0, sym.stream>>>(first, w, ref);
          if (nT) {
            hipk::solveGemvBlockL<BT><<<grid(nT), 256, 0, sym.stream>>>(
                first, last, w, plan.rowGlobal.as<int32_t>(), ref);
          }
        } else {
          if (nT) {
            hipk::solveGemvBlockLt<BT><<<grid(nT), 256, 0, sym.stream>>>(
                first, last, w, plan.rowGlobal.as<int32_t>(), ref);
          }
          hipk::solveTriBlock<BT, true><<<grid(1), 256, 0, sym.stream>>>(first, w, ref);
        }
        continue;
      }
      const LevelRange& lr = levels[item.l];
      const unsigned nP = (unsigned)(lr.panelEnd - lr.panelBegin);
      const unsigned nT = (unsigned)(lr.trsmEnd - lr.trsmBegin);
      if (!nP) continue;
      const dim3 gP = grid(nP), gT = grid(nT);
      if (!BACKWARD) {
        hipk::solveTriPanel<BT, false><<<gP, 256, 0, sym.stream>>>(
            plan.panels.as<PanelDesc>(), plan.levelPanels.as<int32_t>() + lr.panelBegin, ref);
        if (nT) {
          hipk::solveGemvL<BT><<<gT, 256, 0, sym.stream>>>(
              plan.panels.as<PanelDesc>(), plan.trsmTasks.as<TrsmTask>() + lr.trsmBegin,
              plan.rowGlobal.as<int32_t>(), ref);
        }
      } else {
        if (nT) {
          hipk::solveGemvLt<BT><<<gT, 256, 0, sym.stream>>>(
              plan.panels.as<PanelDesc>(), plan.trsmTasks.as<TrsmTask>() + lr.trsmBegin,
              plan.rowGlobal.as<int32_t>(), ref);
        }
        hipk::solveTriPanel<BT, true><<<gP, 256, 0, sym.stream>>>(
            plan.panels.as<PanelDesc>(), plan.levelPanels.as<int32_t>() + lr.panelBegin, ref);
      }
    }
  }

  // single matrix: the pointers themselves; batch: the two pointer arrays, uploaded per call
  hipk::SolveRef<BT> makeRef(const T* data, T* C, int64_t ldc);

  virtual void solveLRange(const T* data, int64_t startLump, int64_t upToLump, T* C,
                           int64_t ldc) override {
    DevPlan& plan = sym.planFor(sym.sparseElimRanges, startLump, upToLump, /*tag=*/0);
    hipk::SolveRef<BT> ref = makeRef(data, C, ldc);
    for (const ElimRangePlan& er : plan.host.elimRanges) elimRange<false>(plan, er, ref);
    denseLevels<false>(plan, plan.host.levels, ref);
    hipCHECK(hipGetLastError());
  }

  virtual void solveLtRange(const T* data, int64_t startLump, int64_t upToLump, T* C,
                            int64_t ldc) override {
    DevPlan& plan = sym.planFor(sym.sparseElimRanges, startLump, upToLump, /*tag=*/0);
    hipk::SolveRef<BT> ref = makeRef(data, C, ldc);
    denseLevels<true>(plan, plan.host.levels, ref);
    for (auto it = plan.host.elimRanges.rbegin(); it != plan.host.elimRanges.rend(); ++it) {
      elimRange<true>(plan, *it, ref);
    }
    hipCHECK(hipGetLastError());
  }

  virtual void addMvRange(const T* data, int64_t startLump, int64_t upToLump, const T* in,
                          int64_t inStride, T* out, int64_t outStride, BaseType<T> alpha) override {
    addMvImpl(data, startLump, upToLump, in, inStride, out, outStride, alpha);
  }
  // (single-matrix types only; the batch types have no addMvFrom in the reference either)
  void addMvImpl(const BT* data, int64_t startLump, int64_t upToLump, const BT* in,
                 int64_t inStride, BT* out, int64_t outStride, BT alpha) {
    const CoalescedBlockMatrixSkel& sk = sym.skel;
    // (lump, row tile) list of the range: built and uploaded once per range, kept by the Solver
    auto& ent = sym.sol.addMvTileLists[{startLump, upToLump}];
    if (!ent.first) {
      vector<int64_t> tiles;
      for (int64_t l = startLump; l < upToLump; l++) {
        const int64_t c0 = sk.chainColPtr[l], nCh = sk.chainColPtr[l + 1] - c0;
        const int64_t rows = sk.chainRowsTillEnd[c0 + nCh - 1];
        const int64_t n = sk.lumpStart[l + 1] - sk.lumpStart[l];
        for (int64_t r = 0; r < rows; r += kTile) {
          for (int64_t c = 0; c < n; c += hipk::kMvCols) {
            if (r < n && c > r + kTile - 1) break;  // entirely above the diagonal
            tiles.push_back(l);
            tiles.push_back(r);
            tiles.push_back(c);
          }
        }
      }
      ent.first.reset(new DevBuf);
      ent.first->upload(tiles);
      ent.second = tiles.size() / 3;
    }
    if (ent.second == 0) return;
    hipk::addMvKernel<BT><<<dim3((unsigned)ent.second, (unsigned)nRHS), 256, 0, sym.stream>>>(
        sym.skelDev(), ent.first->as<int64_t>(), data, in, inStride, out, outStride, alpha);
    hipCHECK(hipGetLastError());
  }
  template <typename V>
  void addMvImpl(const vector<V*>*, int64_t, int64_t, const vector<V*>*, int64_t, vector<V*>*,
                 int64_t, V) {
    throw std::runtime_error("HIP backend: addMvFrom is defined for single matrices only");
  }

  // ---- per-op boundary (MatOps.h:139-168; reference kernels MatOpsCuda.cu:836-1181).  solve() never
  // goes through these (fused path); they exist so that a driver written against the reference's
  // SolveCtx -- the op-by-op loops of Solver.cpp:303-328,357-381,419-448, kept in solver.cpp -- runs
  // on this backend.  Correct, not fast: the dense triangular solves build a one-off device plan.
  hipk::SolveRef<BT> matOnly(const T* data) { return refOf(data, (T*)nullptr, 0); }
  hipk::SolveRef<BT> vecOnly(const T* v, int64_t ld) { return refOf((const T*)nullptr, const_cast<T*>(v), ld); }
  hipk::SolveRef<BT> refOf(const BT* data, BT* C, int64_t ldc) { return {data, C, nullptr, nullptr, ldc}; }
  template <typename V>
  hipk::SolveRef<V> refOf(const vector<V*>* data, vector<V*>* C, int64_t ldc) {
    hipk::SolveRef<V> r{nullptr, nullptr, nullptr, nullptr, ldc};
    if (data) {
      BASPACHO_CHECK_EQ((int)data->size(), batch);
      r.mats = (const V* const*)sym.fac.ptrRing.push(data->data(), data->size() * sizeof(V*), sym.stream);
    }
    if (C) {
      BASPACHO_CHECK_EQ((int)C->size(), batch);
      r.vecs = (V* const*)sym.fac.ptrRing.push(C->data(), C->size() * sizeof(V*), sym.stream);
    }
    return r;
  }
  BT* tmpBuf() {  // order x nRHS values per batch entry, as CpuBaseSolveCtx::tmpBuf
    tmp.resize((size_t)tmpStride() * batch * sizeof(BT));
    return const_cast<BT*>(tmp.as<BT>());
  }
  int64_t tmpStride() const { return sym.skel.order() * nRHS; }

  virtual void sparseElimSolveL(const SymElimCtx& elimData, const T* data, int64_t lumpsBegin,
                                int64_t lumpsEnd, T* C, int64_t ldc) override {
    const HipSymElimCtx* e = dynamic_cast<const HipSymElimCtx*>(&elimData);
    BASPACHO_CHECK_NOTNULL(e);
    BASPACHO_CHECK_EQ(e->lumpsBegin, lumpsBegin);
    BASPACHO_CHECK_EQ(e->lumpsEnd, lumpsEnd);
    DevPlan& plan = sym.planFor({lumpsBegin, lumpsEnd}, lumpsBegin, lumpsEnd, /*tag=*/1);
    hipk::SolveRef<BT> ref = makeRef(data, C, ldc);
    for (const ElimRangePlan& er : plan.host.elimRanges) elimRange<false>(plan, er, ref);
    hipCHECK(hipGetLastError());
  }
  virtual void sparseElimSolveLt(const SymElimCtx& elimData, const T* data, int64_t lumpsBegin,
                                 int64_t lumpsEnd, T* C, int64_t ldc) override {
    const HipSymElimCtx* e = dynamic_cast<const HipSymElimCtx*>(&elimData);
    BASPACHO_CHECK_NOTNULL(e);
    BASPACHO_CHECK_EQ(e->lumpsBegin, lumpsBegin);
    BASPACHO_CHECK_EQ(e->lumpsEnd, lumpsEnd);
    DevPlan& plan = sym.planFor({lumpsBegin, lumpsEnd}, lumpsBegin, lumpsEnd, /*tag=*/1);
    hipk::SolveRef<BT> ref = makeRef(data, C, ldc);
    for (auto it = plan.host.elimRanges.rbegin(); it != plan.host.elimRanges.rend(); ++it) {
      elimRange<true>(plan, *it, ref);
    }
    hipCHECK(hipGetLastError());
  }

  virtual void symm(const T* data, int64_t offset, int64_t n, const T* C, int64_t offC, int64_t ldc,
                    T* D, int64_t ldd, BaseType<T> alpha) override {
    if (n <= 0) return;
    hipk::perOpSymm<BT><<<grid((unsigned)((n + 3) / 4)), 256, 0, sym.stream>>>(
        matOnly(data), offset, n, vecOnly(C, ldc), offC, vecOnly(D, ldd), alpha);
    hipCHECK(hipGetLastError());
  }

  // dense triangular solve with the n x n block at `offset`: the block's panels and row tiles as a
  // one-off plan (the same kernels as the fused path, panel by panel)
  template <bool BACKWARD>
  void denseTriSolve(const T* data, int64_t offset, int64_t n, T* C, int64_t offC, int64_t ldc) {
    if (n <= 0) return;
    opPlans.emplace_back(new DevPlan);
    DevPlan& plan = *opPlans.back();
    plan.host = buildDenseOpPlan(n, 0, offset, /*potrfOnly=*/true, /*vecOff=*/offC);
    vector<LevelRange> levels = plan.host.levels;  // (upload() keeps the level table)
    plan.upload();
    {
      FlagOff noBlocks(sym.blockSolve);  // (the block kernels expect the chain flags of a factor plan)
      denseLevels<BACKWARD>(plan, levels, makeRef(data, C, ldc));
    }
    hipCHECK(hipGetLastError());
  }
  virtual void solveL(const T* data, int64_t offset, int64_t n, T* C, int64_t offC,
                      int64_t ldc) override {
    denseTriSolve<false>(data, offset, n, C, offC, ldc);
  }
  virtual void solveLt(const T* data, int64_t offset, int64_t n, T* C, int64_t offC,
                       int64_t ldc) override {
    denseTriSolve<true>(data, offset, n, C, offC, ldc);
  }

  virtual void gemv(const T* data, int64_t offset, int64_t nRows, int64_t nCols, const T* A,
                    int64_t offA, int64_t lda, BaseType<T> alpha) override {
    if (nRows <= 0) return;
    BASPACHO_CHECK_LE(nRows, sym.skel.order());
    hipk::perOpGemv<BT><<<grid((unsigned)((nRows + 3) / 4)), 256, 0, sym.stream>>>(
        matOnly(data), offset, nRows, nCols, vecOnly(A, lda), offA, alpha, tmpBuf(), tmpStride(), nRHS);
    hipCHECK(hipGetLastError());
  }
  virtual void gemvT(const T* data, int64_t offset, int64_t nRows, int64_t nCols, T* A,
                     int64_t offA, int64_t lda, BaseType<T> alpha) override {
    if (nRows <= 0 || nCols <= 0) return;
    const int64_t colTiles = (nCols + 63) / 64;
    const int64_t rowChunks = (nRows + hipk::kPerOpRowChunk - 1) / hipk::kPerOpRowChunk;
    hipk::perOpGemvT<BT><<<grid((unsigned)(colTiles * rowChunks)), 256, 0, sym.stream>>>(
        matOnly(data), offset, nRows, nCols, vecOnly(A, lda), offA, alpha, tmpBuf(), tmpStride(), nRHS);
    hipCHECK(hipGetLastError());
  }
  virtual void assembleVec(int64_t chainColPtr, int64_t numColItems, T* C, int64_t ldc) override {
    if (numColItems <= 0) return;
    hipk::perOpAssembleVec<BT, false><<<grid((unsigned)numColItems), 256, 0, sym.stream>>>(
        sym.skelDev(), chainColPtr, vecOnly(C, ldc), tmpBuf(), tmpStride(), nRHS);
    hipCHECK(hipGetLastError());
  }
  virtual void assembleVecT(const T* C, int64_t ldc, int64_t chainColPtr,
                            int64_t numColItems) override {
    if (numColItems <= 0) return;
    hipk::perOpAssembleVec<BT, true><<<grid((unsigned)numColItems), 256, 0, sym.stream>>>(
        sym.skelDev(), chainColPtr, vecOnly(C, ldc), tmpBuf(), tmpStride(), nRHS);
    hipCHECK(hipGetLastError());
  }

  // ---- fragmented ops (MatOps.h:170-184, MatOpsFast.cpp:613-1018): whole MV / L / L^T sweeps over
  // a range of spans that are lumps of their own, one right-hand side, contiguous vector.  On this
  // backend they are the fused range kernels (a range of unmerged lumps is just a range).
  virtual bool hasFragmentedOps() override { return true; }
  virtual void fragmentedMV(const T* data, const T* x, int64_t spanBegin, int64_t spanEnd, T* y,
                            BaseType<T> alpha) override {
    checkFragmented(spanBegin, spanEnd);
    addMvImpl(data, spanBegin, spanEnd, x, sym.skel.order(), y, sym.skel.order(), alpha);
  }
  virtual void fragmentedSolveL(const T* data, int64_t spanBegin, int64_t spanEnd, T* y) override {
    checkFragmented(spanBegin, spanEnd);
    solveLRange(data, spanBegin, spanEnd, y, sym.skel.order());
  }
  virtual void fragmentedSolveLt(const T* data, int64_t spanBegin, int64_t spanEnd, T* y) override {
    checkFragmented(spanBegin, spanEnd);
    solveLtRange(data, spanBegin, spanEnd, y, sym.skel.order());
  }
  void checkFragmented(int64_t spanBegin, int64_t spanEnd) const {
    BASPACHO_CHECK_EQ(nRHS, 1);
    BASPACHO_CHECK_LE(spanBegin, spanEnd);
    BASPACHO_CHECK_LE(spanEnd, sym.skel.numLumps());
    // spans in the range are lumps of their own (Solver.cpp:299,352,413)
    BASPACHO_CHECK_EQ(sym.skel.lumpToSpan[spanBegin], spanBegin);
    BASPACHO_CHECK_EQ(sym.skel.lumpToSpan[spanEnd] - sym.skel.lumpToSpan[spanBegin], spanEnd - spanBegin);
  }

  HipSymbolicCtx& sym;
  int nRHS, batch;
  const SolveInvList* invCacheList = nullptr;  // inverses this context computed last (denseLevels)
  uint64_t invCacheGen = 0;
  DevBuf tmp;
  vector<std::unique_ptr<DevPlan>> opPlans;
};

template <>
hipk::SolveRef<double> HipSolveCtx<double>::makeRef(const double* data, double* C, int64_t ldc) {
  return {data, C, nullptr, nullptr, ldc};
}
template <>
hipk::SolveRef<float> HipSolveCtx<float>::makeRef(const float* data, float* C, int64_t ldc) {
  return {data, C, nullptr, nullptr, ldc};
}
template <>
hipk::SolveRef<double> HipSolveCtx<vector<double*>>::makeRef(const vector<double*>* data,
                                                             vector<double*>* C, int64_t ldc) {
  return refOf(data, C, ldc);
}
template <>
hipk::SolveRef<float> HipSolveCtx<vector<float*>>::makeRef(const vector<float*>* data,
                                                           vector<float*>* C, int64_t ldc) {
  return refOf(data, C, ldc);
}

}  // namespace

SolveCtxBase* hipb::createHipSolveCtx(HipSymbolicCtx& sym, std::type_index tIdx, int nRHS, int batch) {
  if (tIdx == std::type_index(typeid(double))) return new HipSolveCtx<double>(sym, nRHS, 1);
  if (tIdx == std::type_index(typeid(float))) return new HipSolveCtx<float>(sym, nRHS, 1);
  if (tIdx == std::type_index(typeid(vector<double*>))) {
    return new HipSolveCtx<vector<double*>>(sym, nRHS, batch);
  }
  if (tIdx == std::type_index(typeid(vector<float*>))) {
    return new HipSolveCtx<vector<float*>>(sym, nRHS, batch);
  }
  return nullptr;
}

int hipBackendReadSweepTrace(SymbolicCtx& sym, long long* out, int maxBlocks) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  if (!h->sol.sweepTrace.ptr) return 0;
  hipCHECK(hipDeviceSynchronize());
  const int n = std::min(maxBlocks, 4096);
  hipCHECK(hipMemcpy(out, h->sol.sweepTrace.ptr, (size_t)n * 4 * sizeof(long long), hipMemcpyDeviceToHost));
  return n;
}


}  // namespace BaSpaCho
