// MI355X backend, the extension operations of hip_backend.h: selected inversion and its adjoint,
// log-det and gradients on the pattern of L, factor status and damping, the reverse-mode sweep of the
// factor, the dense Schur complement, assembly of coordinate entries, normal equations, products
// with a matrix given as entries, matrix-free least squares and products with the factor.  Every
// entry point stages its pointer arguments, splits the batch into chunks and enqueues the launches
// of a chunk on the execution stream (the call path: HipSymbolicCtx::stage / forChunks).
#include "hip_context.h"
#include "hip_cg_kernels.h"
#include "hip_cgls_kernels.h"
#include "hip_chol_adjoint_kernels.h"
#include "hip_factor_product.h"
#include "hip_grad_kernels.h"
#include "hip_lanczos_kernels.h"
#include "hip_norm_est_kernels.h"
#include "hip_ordered_sum.h"
#include "hip_reach_kernels.h"
#include "hip_schur_kernels.h"
#include "hip_selinv_adjoint_kernels.h"
#include "hip_selinv_kernels.h"
#include "hip_status_kernels.h"
#include "jac_product.h"
#include "jac_schur.h"
#include "normal_eq.h"
#include "sym_product.h"

namespace BaSpaCho {

using std::vector;
using namespace hipb;

// the tables of an entry map on the device (entry_map.h), owned by the map.  A host table is uploaded
// by the first call that asks for it and found again by its address inside the map
struct HipEntryMapDev {
  std::map<const void*, DevBuf> tables;
  template <typename U>
  const U* get(const vector<U>& v) {
    auto it = tables.find(&v);
    if (it == tables.end()) {
      DevBuf b;
      b.upload(v);
      it = tables.emplace(&v, std::move(b)).first;
    }
    return it->second.template as<U>();
  }
  static HipEntryMapDev& of(HipEntryMapDevPtr& dev) {
    if (!dev) dev.reset(new HipEntryMapDev);
    return *dev;
  }
};
void hipBackendFreeEntryMap(HipEntryMapDev* dev) { delete dev; }

namespace {

// work lists of the gradient kernels (hip_grad_kernels.h), built once per structure: the patternGrad
// tiles of every lump column and, for logDet's first pass, the lump of the first diagonal element of
// every workgroup.  `part` holds logDet's partial sums, nParts per matrix of a chunk; `statPart` the
// partial records of factorStatus (hip_status_kernels.h), which reads the same firstLump table.
struct GradDev {
  DevBuf tiles, firstLump, part, statPart;
  int64_t nTiles = 0, nParts = 0, partSlices = 0, statSlices = 0;
  vector<int64_t> lumpFirstTile;  // host: first tile of every lump (tiles never cross lumps), then nTiles
  void build(const CoalescedBlockMatrixSkel& sk) {
    vector<hipk::GradTile> tl;
    const int64_t nLumps = sk.numLumps();
    lumpFirstTile.clear();
    for (int64_t l = 0; l < nLumps; l++) {
      lumpFirstTile.push_back((int64_t)tl.size());
      const int64_t w = sk.lumpStart[l + 1] - sk.lumpStart[l];
      const int64_t cBeg = sk.chainColPtr[l], cEnd = sk.chainColPtr[l + 1];
      const int64_t R = sk.chainRowsTillEnd[cEnd - 1], base = sk.chainData[cBeg];
      for (int64_t c0 = 0; c0 < w; c0 += hipk::kGradCols) {
        const int64_t nc = std::min<int64_t>(hipk::kGradCols, w - c0);
        const int64_t trMax = std::min<int64_t>(hipk::kGradRows, std::max<int64_t>(1, hipk::kGradElems / nc));
        int64_t chain = cBeg;
        for (int64_t r0 = 0; r0 < R; r0 += trMax) {
          const int64_t nr = std::min(trMax, R - r0);
          while (sk.chainRowsTillEnd[chain] <= r0) chain++;
          int64_t last = chain;
          while (sk.chainRowsTillEnd[last] < r0 + nr) last++;
          hipk::GradTile t{};
          t.off = base + r0 * w + c0;
          t.lump = (int32_t)l;
          t.r0 = (int32_t)r0;
          t.c0 = (int32_t)c0;
          t.nr = (int32_t)nr;
          t.nc = (int32_t)nc;
          t.chain = (int32_t)chain;
          t.chainEnd = (int32_t)(last + 1);
          tl.push_back(t);
        }
      }
    }
    nTiles = (int64_t)tl.size();
    lumpFirstTile.push_back(nTiles);
    tiles.upload(tl);
    const int64_t n = sk.order();
    nParts = (n + hipk::kLogDetChunk - 1) / hipk::kLogDetChunk;
    vector<int32_t> fl;
    int64_t l = 0;
    for (int64_t b = 0; b < nParts; b++) {
      while (sk.lumpStart[l + 1] <= b * hipk::kLogDetChunk) l++;
      fl.push_back((int32_t)l);
    }
    fl.push_back((int32_t)std::max<int64_t>(nLumps - 1, 0));
    firstLump.upload(fl);
  }
  // room for the partial sums of n matrices.  Growing waits for the kernels queued by earlier calls
  // (they may still use the old buffer); a warm solver does not grow again
  void reservePart(int64_t n) {
    if (n <= partSlices) return;
    if (partSlices > 0) hipCHECK(hipDeviceSynchronize());
    partSlices = 0;
    part.release();
    part.resize((size_t)std::max<int64_t>(nParts * n, 1) * sizeof(double));
    partSlices = n;
  }
  // the same for the partial records of factorStatus
  void reserveStat(int64_t n) {
    if (n <= statSlices) return;
    if (statSlices > 0) hipCHECK(hipDeviceSynchronize());
    statSlices = 0;
    statPart.release();
    statPart.resize((size_t)std::max<int64_t>(nParts * n, 1) * sizeof(hipk::StatusPart));
    statSlices = n;
  }
};

// Scratch of the selected-inversion plans of one structure (the complete plan and the plans up to a
// lump of section 16 share it; it grows to the largest).  Per-matrix slices of a plan's element counts,
// matrix q of a batch chunk in slice q (hipk::SelInvStrides, counted in elements of T).  The buffers are
// sized in fp64: the fp32 slices, half as many bytes each, are packed into the first half of every buffer
struct SelInvScratch {
  DevBuf linv, dd, U, P, Wp;
  int64_t linvCap = 0, uCap = 0, pCap = 0, wCap = 0;  // fp64 elements allocated
  bool allocated = false;
  void release() {
    allocated = false;
    for (DevBuf* b : {&linv, &dd, &U, &P, &Wp}) b->release();
    linvCap = uCap = pCap = wCap = 0;
  }
  // slices of plan `h` that fit
  int64_t slicesFor(const SelInvPlanHost& h) const {
    if (!allocated) return 0;
    int64_t n = INT64_MAX;
    const auto fit = [&n](int64_t cap, int64_t elems) {
      if (elems > 0) n = std::min(n, cap / elems);
    };
    fit(linvCap, h.linvElems);
    fit(uCap, h.uElems);
    fit(pCap, h.pElems);
    fit(wCap, h.wElems);
    return n;
  }
  // grow the scratch to n slices of plan `h`.  Kernels queued by an earlier call (on any stream) may
  // still use the old buffers: wait for them before freeing (as PtrRing::push does).  No slice counts as
  // usable until all five allocations have succeeded: a failed grow (an allocation that throws) leaves
  // nothing allocated, and the next call allocates again instead of launching on released buffers
  void reserve(const SelInvPlanHost& h, int64_t n) {
    if (n <= slicesFor(h)) return;
    if (allocated) hipCHECK(hipDeviceSynchronize());
    allocated = false;
    for (DevBuf* b : {&linv, &dd, &U, &P, &Wp}) b->release();
    const int64_t lc = std::max(linvCap, h.linvElems * n), uc = std::max(uCap, h.uElems * n);
    const int64_t pc = std::max(pCap, h.pElems * n), wc = std::max(wCap, h.wElems * n);
    linvCap = uCap = pCap = wCap = 0;
    const auto bytes = [](int64_t elems) { return (size_t)std::max<int64_t>(elems, 1) * sizeof(double); };
    linv.resize(bytes(lc));
    dd.resize(bytes(lc));
    U.resize(bytes(uc));
    P.resize(bytes(pc));
    Wp.resize(bytes(wc));
    linvCap = lc, uCap = uc, pCap = pc, wCap = wc;
    allocated = true;
  }
};

// selected-inversion plan (hip_plan.h, SelInvPlanHost) on the device, with the shared scratch
struct SelInvDev {
  SelInvPlanHost host;
  DevBuf smalls, nodes, tiles, zTasks, rowChain, rowLocal, pairOff, pairStr;
  SelInvScratch* scratch = nullptr;
  hipk::SelInvStrides strides() const { return {host.linvElems, host.uElems, host.pElems, host.wElems}; }
  // fp64 bytes of one slice of every scratch buffer
  int64_t sliceBytes() const {
    return (2 * host.linvElems + host.uElems + host.pElems + host.wElems) * (int64_t)sizeof(double);
  }
  int64_t slices() const { return scratch->slicesFor(host); }
  void reserve(int64_t n) { scratch->reserve(host, n); }
  // what a pass over the levels hands to its kernels: the scratch as T, the plan tables, the strides
  template <typename T>
  struct View {
    T *linv, *dd, *U, *P, *Wp;
    const SelInvNode* nodes;
    const int2* tiles;
    const int4* zTasks;
    hipk::SelInvStrides st;
  };
  template <typename T>
  View<T> view() const {
    const auto as = [](const DevBuf& b) { return reinterpret_cast<T*>(b.ptr); };
    return {as(scratch->linv), as(scratch->dd), as(scratch->U), as(scratch->P), as(scratch->Wp),
            nodes.as<SelInvNode>(), tiles.as<int2>(), zTasks.as<int4>(), strides()};
  }
  void upload(SelInvScratch* sc) {
    scratch = sc;
    smalls.upload(host.smalls);
    nodes.upload(host.nodes);
    tiles.upload(host.tiles);
    zTasks.upload(host.zTasks);
    rowChain.upload(host.rowChain);
    rowLocal.upload(host.rowLocal);
    pairOff.upload(host.pairOff);
    pairStr.upload(host.pairStr);
    reserve(1);
  }
};

// Reach solves (hip_reach_kernels.h): the tables of a call travel through a ring
// of their own (a plan is built per call: its queries are the call's), and inverseBlocks keeps its W here.
// The ring is sized for both blobs of a call before the call queues anything (hipBackendReachSolveL), so
// it never grows between the kernels of one call; a call with larger tables than any before waits for the
// device at its beginning, as a larger W does, and 32 slots of the largest blob seen stay pinned.
struct ReachDev {
  PtrRing ring;
  DevBuf W;
  // room for `bytes` of W.  Growing waits for the kernels queued by earlier calls, as the other scratch does
  void* reserve(size_t bytes) {
    if (bytes > W.bytes) {
      if (W.bytes > 0) hipCHECK(hipDeviceSynchronize());
      W.resize(bytes);
    }
    return W.ptr;
  }
};

// Products with the factor (hip_factor_product.h): the plan of the structure on
// the device, and the partial sums of the split strips of y = L^T x, partElems per (member of a chunk,
// right-hand side)
struct FactorProductState {
  FactorProductPlan host;
  DevBuf spanChainPtr, spanChain, spanChainLump, rowToSpan, spanLong, longRows, hugeSpans, hugeWidePtr, hugeWide,
      ltTasks, ltFolds, smallColLump, smallCol, part;
  int64_t partSlabs = 0;
  void build(const CoalescedBlockMatrixSkel& sk) {
    host = buildFactorProductPlan(sk);
    spanChainPtr.upload(host.spanChainPtr);
    spanChain.upload(host.spanChain);
    spanChainLump.upload(host.spanChainLump);
    rowToSpan.upload(host.rowToSpan);
    spanLong.upload(host.spanLong);
    longRows.upload(host.longRows);
    hugeSpans.upload(host.hugeSpans);
    hugeWidePtr.upload(host.hugeWidePtr);
    hugeWide.upload(host.hugeWide);
    ltTasks.upload(host.ltTasks);
    ltFolds.upload(host.ltFolds);
    smallColLump.upload(host.smallColLump);
    smallCol.upload(host.smallCol);
  }
  hipk::FactorProductDev dev() const {
    return {spanChainPtr.as<int32_t>(), spanChain.as<int32_t>(), spanChainLump.as<int32_t>(),
            rowToSpan.as<int32_t>(),    spanLong.as<int32_t>(),  longRows.as<int32_t>(),
            hugeSpans.as<int32_t>(),    hugeWidePtr.as<int32_t>(), hugeWide.as<int32_t>(),
            ltTasks.as<LtTask>(),       ltFolds.as<LtFold>(),    smallColLump.as<int32_t>(),
            smallCol.as<int32_t>()};
  }
  // room for the partial sums of n (member, right-hand side) pairs, sized in fp64.  Growing waits for
  // the kernels queued by earlier calls, as the other scratch does
  void reservePart(int64_t n) {
    if (n <= partSlabs || host.partElems == 0) return;
    if (partSlabs > 0) hipCHECK(hipDeviceSynchronize());
    partSlabs = 0;
    part.release();
    part.resize((size_t)(host.partElems * n) * sizeof(double));
    partSlabs = n;
  }
};

// several host tables as one blob, every table at a multiple of 16 bytes
struct TableBlob {
  vector<char> bytes;
  // the size of a blob of `size` bytes after add(v)
  template <typename U>
  static size_t sizeWith(size_t size, const vector<U>& v) {
    return ((size + 15) & ~size_t(15)) + v.size() * sizeof(U);
  }
  template <typename U>
  size_t add(const vector<U>& v) {
    const size_t off = (bytes.size() + 15) & ~size_t(15);
    bytes.resize(sizeWith(bytes.size(), v));
    if (!v.empty()) std::memcpy(bytes.data() + off, v.data(), v.size() * sizeof(U));
    return off;
  }
};

}  // namespace

// the extension state of a context (HipSymbolicCtx::ext), built on first use
struct hipb::ExtensionState {
  std::unique_ptr<SelInvDev> selinv;  // selected-inversion plan, built on first use
  std::map<int64_t, std::unique_ptr<SelInvDev>> selinvUpTo;  // ... up to a lump, per cut
  SelInvScratch selinvScratch;
  std::unique_ptr<GradDev> grad;      // work lists of logDet / patternGrad, built on first use
  ReachDev reach;
  std::unique_ptr<FactorProductState> factorProduct;  // plan of mulL / mulLt, built on first use
  // partials of maxRatio / colMax (hip_norm_est_kernels.h).  Growing waits for the kernels queued by
  // earlier calls, as GradDev::reservePart does; a warm solver does not grow again
  DevBuf redPart;
  int64_t redParts = 0;
  hipk::RedPart* reserveRedParts(int64_t n) {
    if (n > redParts) {
      if (redParts > 0) hipCHECK(hipDeviceSynchronize());
      redParts = 0;
      redPart.release();
      redPart.resize((size_t)std::max<int64_t>(n, 1) * sizeof(hipk::RedPart));
      redParts = n;
    }
    return reinterpret_cast<hipk::RedPart*>(redPart.ptr);
  }
};
void hipb::ExtensionStateDelete::operator()(ExtensionState* p) const { delete p; }

namespace {

HipSymbolicCtx& hipCtx(SymbolicCtx& sym) {
  HipSymbolicCtx* h = dynamic_cast<HipSymbolicCtx*>(&sym);
  BASPACHO_CHECK_NOTNULL(h);
  return *h;
}

ExtensionState& extState(HipSymbolicCtx& h) {
  if (!h.ext) h.ext.reset(new ExtensionState);
  return *h.ext;
}

// ---- gradients on the pattern of L (hip_grad_kernels.h) -------------------
GradDev& gradPlan(HipSymbolicCtx& h) {
  ExtensionState& x = extState(h);
  const CoalescedBlockMatrixSkel& skel = h.skel;
  if (!x.grad) {
    std::unique_ptr<GradDev> p(new GradDev);
    p->build(skel);
    x.grad = std::move(p);
  }
  return *x.grad;
}

// matrices per chunk of a batched pass over plan `d`, with the scratch grown to it: min(batch, 65535
// (gridDim.y), what half the free device memory holds in slices -- slices already held count as
// free), at least 1, at most the testing cap
int64_t selInvChunk(HipSymbolicCtx& h, SelInvDev& d, int64_t batch) {
  int64_t chunk = std::min(batch, HipSymbolicCtx::kMaxGridY);
  if (h.selInvChunkCap > 0) chunk = std::min<int64_t>(chunk, h.selInvChunkCap);
  const int64_t slice = d.sliceBytes();
  if (chunk > d.slices() && slice > 0) {
    size_t freeBytes = 0, totalBytes = 0;
    hipCHECK(hipMemGetInfo(&freeBytes, &totalBytes));
    const int64_t fit = std::max<int64_t>(d.slices(), (int64_t)(freeBytes / 2) / slice);
    chunk = std::max<int64_t>(1, std::min(chunk, fit));
  }
  d.reserve(chunk);
  return chunk;
}

SelInvDev& selInvPlan(HipSymbolicCtx& h) {
  ExtensionState& x = extState(h);
  const CoalescedBlockMatrixSkel& skel = h.skel;
  if (!x.selinv) {
    std::unique_ptr<SelInvDev> p(new SelInvDev);
    p->host = buildSelInvPlan(skel);
    p->upload(&x.selinvScratch);
    x.selinv = std::move(p);
  }
  return *x.selinv;
}

// the plan of the lumps < upToLump (section 16), cached per cut beside the complete one, as planFor
// caches factor plans; all of them work in the one scratch
SelInvDev& selInvPlanUpTo(HipSymbolicCtx& h, int64_t upToLump) {
  ExtensionState& x = extState(h);
  const CoalescedBlockMatrixSkel& skel = h.skel;
  if (upToLump == skel.numLumps()) return selInvPlan(h);
  std::unique_ptr<SelInvDev>& slot = x.selinvUpTo[upToLump];
  if (!slot) {
    std::unique_ptr<SelInvDev> p(new SelInvDev);
    p->host = buildSelInvPlan(skel, upToLump);
    p->upload(&x.selinvScratch);
    slot = std::move(p);
  }
  return *slot;
}

// one pass over the levels for `nMats` matrices (gridDim.y), in scratch slices 0 .. nMats-1
template <typename T>
void selInvLevels(HipSymbolicCtx& h, const SelInvDev& d, hipk::DataRef<T> data, unsigned nMats) {
  const hipStream_t stream = h.stream;
  HipRunCounters& counters = h.counters;
  const hipk::SkelDev sk = h.skelDev();
  const SelInvDev::View<T> w = d.view<T>();
  int64_t launches = 0;
  for (const SelInvLevel& L : d.host.levels) {
    if (L.smallEnd > L.smallBegin) {
      hipk::selinvSmallLumps<T><<<dim3((unsigned)(L.smallEnd - L.smallBegin), nMats), 64, 0, stream>>>(
          d.smalls.as<SelInvSmall>() + L.smallBegin, sk, data);
      launches++;
    }
    const unsigned nNodes = (unsigned)(L.nodeEnd - L.nodeBegin);
    if (nNodes == 0) continue;
    const SelInvNode* nd = w.nodes + L.nodeBegin;
    hipk::selinvDiagInverse<T><<<dim3(nNodes, nMats), 256, 0, stream>>>(nd, data, w.linv, w.dd, w.st);
    const unsigned nTiles = (unsigned)(L.tileEnd - L.tileBegin);
    if (nTiles > 0) {
      hipk::selinvFormU<T><<<dim3(nTiles, nMats), 256, 0, stream>>>(nd, w.tiles + L.tileBegin, data, w.linv, w.U,
                                                                    w.st);
      hipk::selinvZrrTimesU<T><<<dim3((unsigned)(L.zEnd - L.zBegin), nMats), 256, 0, stream>>>(
          nd, w.zTasks + L.zBegin, d.rowChain.as<int32_t>(), d.rowLocal.as<int32_t>(),
          d.pairOff.as<int64_t>(), d.pairStr.as<int32_t>(), data, w.U, w.P, w.st);
      hipk::selinvReduceZ<T><<<dim3(nTiles, nMats), 256, 0, stream>>>(nd, w.tiles + L.tileBegin, data, w.U, w.P,
                                                                      w.Wp, w.st);
      launches += 3;
    }
    hipk::selinvDiagBlock<T><<<dim3(nNodes, nMats), 256, 0, stream>>>(nd, data, w.dd, w.Wp, w.st);
    launches += 2;
  }
  counters.selinvLaunches += launches;
  counters.selinvChunks++;
}

// one right-to-left pass over the selected-inversion levels for `nMats` matrices (gridDim.y), in
// scratch slices 0 .. nMats-1.  selinvDiagInverse and selinvZrrTimesU run as they are: the first
// reads L (it does not write its data), the second multiplies G_RR by the copy of L_RI in U.
template <typename T>
void cholAdjLevels(HipSymbolicCtx& h, const SelInvDev& d, hipk::DataRef<const T> lref, hipk::DataRef<T> gref,
                   unsigned nMats) {
  const hipStream_t stream = h.stream;
  const hipk::SkelDev sk = h.skelDev();
  const SelInvDev::View<T> w = d.view<T>();
  const hipk::DataRef<T> lmut{const_cast<T*>(lref.single), const_cast<T* const*>(lref.many)};
  for (const SelInvLevel& L : d.host.levels) {
    if (L.smallEnd > L.smallBegin) {
      hipk::cholAdjSmallLumps<T><<<dim3((unsigned)(L.smallEnd - L.smallBegin), nMats), 64, 0, stream>>>(
          d.smalls.as<SelInvSmall>() + L.smallBegin, sk, lref, gref);
    }
    const unsigned nNodes = (unsigned)(L.nodeEnd - L.nodeBegin);
    if (nNodes == 0) continue;
    const SelInvNode* nd = w.nodes + L.nodeBegin;
    hipk::selinvDiagInverse<T><<<dim3(nNodes, nMats), 256, 0, stream>>>(nd, lmut, w.linv, w.dd, w.st);
    const unsigned nTiles = (unsigned)(L.tileEnd - L.tileBegin);
    if (nTiles > 0) {
      hipk::cholAdjGatherL<T><<<dim3(nTiles, nMats), 256, 0, stream>>>(nd, w.tiles + L.tileBegin, lref, w.U, w.st);
      hipk::selinvZrrTimesU<T><<<dim3((unsigned)(L.zEnd - L.zBegin), nMats), 256, 0, stream>>>(
          nd, w.zTasks + L.zBegin, d.rowChain.as<int32_t>(), d.rowLocal.as<int32_t>(),
          d.pairOff.as<int64_t>(), d.pairStr.as<int32_t>(), gref, w.U, w.P, w.st);
      hipk::cholAdjReduce<T><<<dim3(nTiles, nMats), 256, 0, stream>>>(nd, w.tiles + L.tileBegin, gref, w.linv, w.U,
                                                                      w.P, w.Wp, w.st);
    }
    hipk::cholAdjDiag<T><<<dim3(nNodes, nMats), 256, 0, stream>>>(nd, lref, gref, w.linv, w.Wp, w.st);
  }
}

// one pass over the selected-inversion levels, last level first, for `nMats` matrices (gridDim.y), in
// scratch slices 0 .. nMats-1.  selinvDiagInverse and selinvZrrTimesU run as they are: the first reads
// L, the second multiplies Z_RR by the S_RI that selinvAdjStage left in U (neither writes its data).
// A level of one node has one writer per slot of the scatter: no atomics there.
template <typename T>
void selInvAdjLevels(HipSymbolicCtx& h, const SelInvDev& d, hipk::DataRef<const T> lref, hipk::DataRef<const T> zref,
                     hipk::DataRef<T> gref, unsigned nMats) {
  const hipStream_t stream = h.stream;
  HipRunCounters& counters = h.counters;
  const hipk::SkelDev sk = h.skelDev();
  const SelInvDev::View<T> w = d.view<T>();
  const hipk::DataRef<T> lmut{const_cast<T*>(lref.single), const_cast<T* const*>(lref.many)};
  const hipk::DataRef<T> zmut{const_cast<T*>(zref.single), const_cast<T* const*>(zref.many)};
  int64_t launches = 0;
  for (auto it = d.host.levels.rbegin(); it != d.host.levels.rend(); ++it) {
    const SelInvLevel& L = *it;
    if (L.smallEnd > L.smallBegin) {
      hipk::selinvAdjSmallLumps<T><<<dim3((unsigned)(L.smallEnd - L.smallBegin), nMats), 64, 0, stream>>>(
          d.smalls.as<SelInvSmall>() + L.smallBegin, sk, lref, zref, gref);
      launches++;
    }
    const unsigned nNodes = (unsigned)(L.nodeEnd - L.nodeBegin);
    if (nNodes == 0) continue;
    const SelInvNode* nd = w.nodes + L.nodeBegin;
    hipk::selinvDiagInverse<T><<<dim3(nNodes, nMats), 256, 0, stream>>>(nd, lmut, w.linv, w.dd, w.st);
    const unsigned nTiles = (unsigned)(L.tileEnd - L.tileBegin);
    if (nTiles > 0) {
      const unsigned nZ = (unsigned)(L.zEnd - L.zBegin);
      hipk::selinvAdjStage<T><<<dim3(nTiles, nMats), 256, 0, stream>>>(nd, w.tiles + L.tileBegin, lref, gref, w.linv,
                                                                       w.U, w.P, w.Wp, w.st);
      // workgroups per task: one per 64 source rows of the level's longest chunk, at most 8
      int maxChunk = 0;
      for (int64_t n = L.nodeBegin; n < L.nodeEnd; n++) maxChunk = std::max(maxChunk, (int)d.host.nodes[n].kChunk);
      const dim3 sgrid(nZ, nMats, (unsigned)std::min(8, std::max(1, (maxChunk + 63) / 64)));
      if (nNodes == 1) {
        hipk::selinvAdjScatter<T, false><<<sgrid, 256, 0, stream>>>(
            nd, w.zTasks + L.zBegin, d.rowChain.as<int32_t>(), d.rowLocal.as<int32_t>(), d.pairOff.as<int64_t>(),
            d.pairStr.as<int32_t>(), gref, w.P, w.Wp, w.st);
      } else {
        hipk::selinvAdjScatter<T, true><<<sgrid, 256, 0, stream>>>(
            nd, w.zTasks + L.zBegin, d.rowChain.as<int32_t>(), d.rowLocal.as<int32_t>(), d.pairOff.as<int64_t>(),
            d.pairStr.as<int32_t>(), gref, w.P, w.Wp, w.st);
      }
      hipk::selinvZrrTimesU<T><<<dim3(nZ, nMats), 256, 0, stream>>>(
          nd, w.zTasks + L.zBegin, d.rowChain.as<int32_t>(), d.rowLocal.as<int32_t>(), d.pairOff.as<int64_t>(),
          d.pairStr.as<int32_t>(), zmut, w.U, w.P, w.st);
      hipk::selinvAdjReduce<T><<<dim3(nTiles, nMats), 256, 0, stream>>>(nd, w.tiles + L.tileBegin, lref, zref, gref,
                                                                        w.linv, w.P, w.Wp, w.st);
      launches += 4;
    }
    hipk::selinvAdjDiag<T><<<dim3(nNodes, nMats), 256, 0, stream>>>(nd, gref, w.linv, w.Wp, w.st);
    launches += 2;
  }
  counters.selinvLaunches += launches;
  counters.selinvChunks++;
}

}  // namespace

void hipBackendSetSelInvBatchChunk(SymbolicCtx& sym, int64_t maxMatrices) {
  BASPACHO_CHECK_GE(maxMatrices, 0);
  hipCtx(sym).selInvChunkCap = maxMatrices;
}

int64_t hipBackendPtrRingSlotBytes(SymbolicCtx& sym) { return (int64_t)hipCtx(sym).fac.ptrRing.slotBytes; }

// Selected inversion of `batch` complete factors, in place (hip_selinv_kernels.h).  The plan is built
// and uploaded on the first call; every launch goes to the execution stream, in level order, with no
// host synchronisation.  A chunk is one pass over the levels, each matrix in its own scratch slice;
// the scratch grows to the chunk (selInvChunk) and stays with the solver.
template <typename T>
void hipBackendSelectedInverse(SymbolicCtx& sym, T* const* data, int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  h.checkDevice();
  SelInvDev& d = selInvPlan(h);
  const int64_t chunk = selInvChunk(h, d, batch);
  const BatchPtrs<T> z = h.stage(data, batch, single);
  h.forChunks(batch, chunk, [&](int64_t q0, unsigned nm) { selInvLevels<T>(h, d, z.at(q0), nm); });
}

// ---- reverse mode of selected inversion (hip_selinv_adjoint_kernels.h) -------
// L[q] a complete factor, Z[q] its selected inverse (both read only); grad[q]: the gradient of every
// slot of Z on entry, Lbar on return.  The complete plan, its scratch and its chunks, the levels taken
// from the last to the first.
template <typename T>
void hipBackendSelectedInverseAdjoint(SymbolicCtx& sym, const T* const* L, const T* const* Z, T* const* G,
                                      int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  h.checkDevice();
  SelInvDev& d = selInvPlan(h);
  const int64_t chunk = selInvChunk(h, d, batch);
  const BatchPtrs<const T> l = h.stage(L, batch, single), z = h.stage(Z, batch, single);
  const BatchPtrs<T> gr = h.stage(G, batch, single);
  h.forChunks(batch, chunk, [&](int64_t q0, unsigned nm) { selInvAdjLevels<T>(h, d, l.at(q0), z.at(q0), gr.at(q0), nm); });
}

// logDet of `batch` factors: two launches per chunk, the partial sums of a chunk in GradDev::part
template <typename T>
void hipBackendLogDet(SymbolicCtx& sym, const T* const* factors, int64_t batch, bool single, T* out) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  const CoalescedBlockMatrixSkel& skel = h.skel;
  h.checkDevice();
  GradDev& g = gradPlan(h);
  const hipk::SkelDev sk = h.skelDev();
  const int64_t chunk = std::min(batch, HipSymbolicCtx::kMaxGridY);
  g.reservePart(chunk);
  const BatchPtrs<const T> f = h.stage(factors, batch, single);
  double* part = reinterpret_cast<double*>(g.part.ptr);
  h.forChunks(batch, chunk, [&](int64_t q0, unsigned nm) {
    if (g.nParts > 0) {
      hipk::logDetPartial<T><<<dim3((unsigned)g.nParts, nm), 256, 0, stream>>>(
          sk, g.firstLump.as<int32_t>(), skel.order(), (int)g.nParts, f.at(q0), part);
    }
    hipk::logDetFinal<T><<<dim3(1, nm), 256, 0, stream>>>(part, (int)g.nParts, out + q0);
  });
}

// patternGrad of a.batch matrices: one launch of every tile per chunk
template <typename T>
void hipBackendPatternGrad(SymbolicCtx& sym, const HipGradArgs<T>& a, int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  GradDev& g = gradPlan(h);
  const hipk::SkelDev sk = h.skelDev();
  if (g.nTiles == 0) return;
  const bool hasZ = a.z != nullptr, hasUV = a.u != nullptr;
  const BatchPtrs<const T> z = h.stage(a.z, batch, single);
  const BatchPtrs<const T> u = h.stage(a.u, batch, single), v = h.stage(hasUV ? a.v : nullptr, batch, single);
  const BatchPtrs<T> o = h.stage(a.out, batch, single);
  const int k = hasUV ? a.nRHS : 0;
  const int kc = std::min(k, hipk::kGradK);
  const size_t lds = k > 0 ? (size_t)(hipk::kGradRows + hipk::kGradCols) * (kc + 1) * 2 * sizeof(T) : 0;
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    if (a.outer) {
      hipk::patternGradTiles<T, true><<<dim3((unsigned)g.nTiles, nm), 256, lds, stream>>>(
          g.tiles.as<hipk::GradTile>(), sk, hipk::DataRef<const T>{nullptr, nullptr}, nullptr, u.at(q0), v.at(q0),
          a.ld, k, a.alpha, o.at(q0));
    } else {
      hipk::patternGradTiles<T><<<dim3((unsigned)g.nTiles, nm), 256, lds, stream>>>(
          g.tiles.as<hipk::GradTile>(), sk, z.at(q0), hasZ ? a.zScale + q0 : nullptr, u.at(q0), v.at(q0), a.ld, k,
          a.alpha, o.at(q0));
    }
  });
}

// ---- factor status and damping of the diagonal (hip_status_kernels.h) -------
// the records of `batch` buffers over the internal scalars [g0, g1): two launches per chunk, chunks as
// logDet's, the partial records of a chunk in GradDev::statPart
template <typename T>
void hipBackendFactorStatus(SymbolicCtx& sym, const T* const* data, int64_t batch, bool single, int64_t spanBegin,
                            int64_t spanEnd, int64_t* out) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  const CoalescedBlockMatrixSkel& skel = h.skel;
  h.checkDevice();
  GradDev& g = gradPlan(h);
  const hipk::SkelDev sk = h.skelDev();
  const int64_t g0 = skel.spanStart[spanBegin], g1 = skel.spanStart[spanEnd];
  const int64_t b0 = g0 / hipk::kLogDetChunk;
  const int64_t nParts = g1 > g0 ? (g1 + hipk::kLogDetChunk - 1) / hipk::kLogDetChunk - b0 : 0;
  BASPACHO_CHECK_LE(b0 + nParts, g.nParts);
  const int64_t chunk = std::min(batch, HipSymbolicCtx::kMaxGridY);
  g.reserveStat(chunk);
  const BatchPtrs<const T> d = h.stage(data, batch, single);
  hipk::StatusPart* part = reinterpret_cast<hipk::StatusPart*>(g.statPart.ptr);
  h.forChunks(batch, chunk, [&](int64_t q0, unsigned nm) {
    if (nParts > 0) {
      hipk::factorStatusPartial<T><<<dim3((unsigned)nParts, nm), 256, 0, stream>>>(
          sk, g.firstLump.as<int32_t>(), g0, g1, b0, (int)nParts, d.at(q0), part);
    }
    hipk::factorStatusFinal<<<dim3(1, nm), 256, 0, stream>>>(part, (int)nParts, out + 4 * q0);
  });
}

// diagonal <- diagonal (1 + alpha) + beta on the internal scalars [g0, g1) of `batch` buffers, alpha
// and beta of member q at ab[2 q], ab[2 q + 1] on the device: one launch per chunk
template <typename T>
void hipBackendDampDiagonal(SymbolicCtx& sym, T* const* data, int64_t batch, bool single, int64_t spanBegin,
                            int64_t spanEnd, const T* ab) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  const CoalescedBlockMatrixSkel& skel = h.skel;
  h.checkDevice();
  GradDev& g = gradPlan(h);
  const hipk::SkelDev sk = h.skelDev();
  const int64_t g0 = skel.spanStart[spanBegin], g1 = skel.spanStart[spanEnd];
  if (g1 <= g0) return;
  const int64_t base = g0 - g0 % 256, wgs = (g1 - base + 255) / 256;
  const BatchPtrs<T> d = h.stage(data, batch, single);
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    hipk::dampDiagonal<T><<<dim3((unsigned)wgs, nm), 256, 0, stream>>>(sk, g.firstLump.as<int32_t>(), g0, g1, base,
                                                                       d.at(q0), ab + 2 * q0);
  });
}

// ---- reverse-mode sweep of the factor (DESIGN.md sections 15 and 16) -----------------------------
// P[q] = factorUpTo of the lumps < upToLump (read only); grad[q]: Lbar before the cut and Sbar behind
// it on entry, the data gradient on return.  Per chunk: seed the trailing lumps, run the plan of the
// cut on the selected-inversion scratch (chunks as selectedInverse), then the final pass over every
// tile.  upToLump = numLumps is the sweep of the complete factor: the complete plan, nothing to seed.
template <typename T>
void hipBackendFactorAdjointUpTo(SymbolicCtx& sym, const T* const* L, T* const* G, int64_t batch, bool single,
                                 int64_t upToLump) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  SelInvDev& d = selInvPlanUpTo(h, upToLump);
  GradDev& g = gradPlan(h);
  const int64_t chunk = selInvChunk(h, d, batch);
  const BatchPtrs<const T> l = h.stage(L, batch, single);
  const BatchPtrs<T> gr = h.stage(G, batch, single);
  const hipk::SkelDev sk = h.skelDev();
  const int64_t seed0 = g.lumpFirstTile[upToLump], nSeed = g.nTiles - seed0;
  h.forChunks(batch, chunk, [&](int64_t q0, unsigned nm) {
    const hipk::DataRef<T> gref = gr.at(q0);
    if (nSeed > 0) {
      hipk::cholAdjSeedTrailing<T><<<dim3((unsigned)nSeed, nm), 256, 0, stream>>>(
          g.tiles.as<hipk::GradTile>() + seed0, sk, gref);
    }
    cholAdjLevels<T>(h, d, l.at(q0), gref, nm);
    if (g.nTiles > 0) {
      hipk::cholAdjFinal<T><<<dim3((unsigned)g.nTiles, nm), 256, 0, stream>>>(g.tiles.as<hipk::GradTile>(), sk,
                                                                             gref);
    }
  });
}

// The trailing block (from the first scalar of lump `fromLump` on) of `batch` layout buffers to dense
// symmetric m x m matrices (toDense), or the adjoint of that in the data-gradient convention
// (!toDense: in = dense gradients, out = layout buffers, written whole).  dest: device permutation of
// 0 .. m-1 or NULL.  One launch per chunk.
template <typename T>
void hipBackendSchurDense(SymbolicCtx& sym, const T* const* in, T* const* out, int64_t batch, bool single,
                          int64_t fromLump, const int32_t* dest, bool toDense) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  const CoalescedBlockMatrixSkel& skel = h.skel;
  h.checkDevice();
  const hipk::SkelDev sk = h.skelDev();
  const int64_t bar = skel.lumpStart[fromLump], m = skel.order() - bar;
  BASPACHO_CHECK_LT(m, (int64_t)INT32_MAX);
  const int64_t nT = (m + hipk::kSchurTile - 1) / hipk::kSchurTile, nPairs = nT * (nT + 1) / 2;
  BASPACHO_CHECK_LT(nPairs, (int64_t)INT32_MAX);
  GradDev* g = toDense ? nullptr : &gradPlan(h);
  const int64_t nWork = toDense ? nPairs : g->nTiles;
  if (nWork == 0) return;
  const BatchPtrs<const T> i = h.stage(in, batch, single);
  const BatchPtrs<T> o = h.stage(out, batch, single);
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    if (toDense) {
      hipk::schurToDense<T><<<dim3((unsigned)nPairs, nm), 256, 0, stream>>>(
          sk, skel.lumpToSpan[fromLump], skel.numSpans(), bar, m, dest, i.at(q0), o.at(q0));
    } else {
      hipk::schurFromDense<T><<<dim3((unsigned)g->nTiles, nm), 256, 0, stream>>>(
          g->tiles.as<hipk::GradTile>(), sk, (int)g->lumpFirstTile[fromLump], bar, m, dest, i.at(q0), o.at(q0));
    }
  });
}

// ---- ordered sums over entry maps (hip_ordered_sum.h, DESIGN.md sections 14, 17 and 21) -----------
namespace {

// the tile kernel over the runs `t` of a map with `numTiles` tiles of `dataSize` layout elements
struct TileLaunch {
  int64_t dataSize, numTiles;
  const int32_t *tileFirst, *tileLongFirst, *runStart;
  const uint16_t* destLocal;
  const int32_t* longDest;
  TileLaunch(HipEntryMapDev& d, const TileRuns& t, int64_t dataSize, int64_t numTiles)
      : dataSize(dataSize), numTiles(numTiles), tileFirst(d.get(t.tileFirst)),
        tileLongFirst(d.get(t.tileLongFirst)), runStart(d.get(t.runStart)), destLocal(d.get(t.destLocal)),
        longDest(d.get(t.longDest)) {}
  template <typename T, typename Term>
  void operator()(hipStream_t stream, const Term& term, hipk::DataRef<T> out, unsigned nm) const {
    hipk::orderedSumTiles<T><<<dim3((unsigned)numTiles, nm), hipk::kAsmThreads, 0, stream>>>(
        dataSize, tileFirst, tileLongFirst, runStart, destLocal, longDest, term, out);
  }
};

// the run kernel over `numRuns` runs and q vectors: one thread per output, then one wave per (long
// run, vector) of the `numLong` runs of longRuns (NULL: no long list, every run by one lane)
template <typename Start>
struct RunLaunch {
  int64_t numRuns, q, shortWgs, longWaves, longWgs;
  const Start* start;
  const int32_t *longRuns, *entry = nullptr, *idx = nullptr;  // entry, idx: those of a RunList
  RunLaunch(int64_t numRuns, int64_t q, const Start* start, const int32_t* longRuns, int64_t numLong)
      : numRuns(numRuns), q(q), shortWgs((numRuns * q + hipk::kAsmThreads - 1) / hipk::kAsmThreads),
        longWaves(numLong * q), longWgs((longWaves + hipk::kAsmWavesPerWg - 1) / hipk::kAsmWavesPerWg),
        start(start), longRuns(longRuns) {
    BASPACHO_CHECK_LT(shortWgs + longWgs, (int64_t)INT32_MAX);
  }
  template <typename T, typename Term>
  void operator()(hipStream_t stream, const Term& term, hipk::DataRef<T> out, unsigned nm) const {
    hipk::orderedSumRuns<T><<<dim3((unsigned)(shortWgs + longWgs), nm), hipk::kAsmThreads, 0, stream>>>(
        numRuns, (int32_t)q, (int32_t)shortWgs, longWaves, start, longRuns, term, out);
  }
};
RunLaunch<int32_t> runLaunch(HipEntryMapDev& d, const RunList& r, int64_t q, bool withLong) {
  RunLaunch<int32_t> l((int64_t)r.start.size() - 1, q, d.get(r.start), withLong ? d.get(r.longRuns) : nullptr,
                       withLong ? (int64_t)r.longRuns.size() : 0);
  l.entry = d.get(r.entry);
  l.idx = d.get(r.idx);
  return l;
}

// stages the operands (b may be NULL) and calls launch(a, b, out, members) for every chunk of the batch
template <typename T, typename Launch>
void forOperandChunks(HipSymbolicCtx& h, const T* const* a, const T* const* b, T* const* out, int64_t batch,
                      bool single, Launch launch) {
  const BatchPtrs<const T> as = h.stage(a, batch, single), bs = h.stage(b, batch, single);
  const BatchPtrs<T> o = h.stage(out, batch, single);
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY,
              [&](int64_t q0, unsigned nm) { launch(as.at(q0), bs.at(q0), o.at(q0), nm); });
}

}  // namespace

// assemble (or its adjoint) of `batch` matrices: one launch per chunk
template <typename T>
void hipBackendAssemble(SymbolicCtx& sym, const AssemblyMap& m, const T* const* in, T* const* out, int64_t batch,
                        bool single, bool adjoint) {
  using In = hipk::DataRef<const T>;
  using Out = hipk::DataRef<T>;
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  // the whole map with the first call, whichever direction it takes
  HipEntryMapDev& d = HipEntryMapDev::of(m.dev);
  const int64_t* entryOff = d.get(m.entryOff);
  const int32_t* runEntry = d.get(m.runEntry);
  const TileLaunch tiles(d, m.tiles, m.dataSize, m.numTiles);
  if (adjoint && m.nnz == 0) return;
  const int64_t per = hipk::kAsmThreads * hipk::kAsmAdjPer;
  forOperandChunks<T>(h, in, nullptr, out, batch, single, [&](In i, In, Out o, unsigned nm) {
    if (adjoint) {
      hipk::assembleAdjointEntries<T><<<dim3((unsigned)((m.nnz + per - 1) / per), nm), hipk::kAsmThreads, 0,
                                         stream>>>(m.nnz, entryOff, i, o);
    } else {
      tiles(stream, hipk::EntryTerm<T>{runEntry, i}, o, nm);
    }
  });
}

// one of the four operations of the normal equations on `batch` members: one launch per chunk
template <typename T>
void hipBackendNormalEq(SymbolicCtx& sym, const NormalEqMap& m, int32_t op, const T* const* values,
                        const T* const* x, T* const* out, int64_t q, int64_t batch, bool single) {
  using In = hipk::DataRef<const T>;
  using Out = hipk::DataRef<T>;
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  HipEntryMapDev& d = HipEntryMapDev::of(m.dev);
  if (op == NormalEqHessian) {
    const TileLaunch tiles(d, m.tiles, m.dataSize, m.numTiles);
    const int32_t *pairA = d.get(m.pairA), *pairB = d.get(m.pairB);
    if (m.numTiles == 0) return;
    forOperandChunks<T>(h, values, x, out, batch, single, [&](In v, In, Out o, unsigned nm) {
      tiles(stream, hipk::PairTerm<T>{pairA, pairB, v}, o, nm);
    });
  } else if (op == NormalEqAdjoint) {
    const RunLaunch<int64_t> runs(m.nnz, 1, d.get(m.adjStart), d.get(m.adjLong), (int64_t)m.adjLong.size());
    const int64_t* adjDest = d.get(m.adjDest);
    const int32_t* adjPartner = d.get(m.adjPartner);
    if (m.nnz == 0) return;
    forOperandChunks<T>(h, values, x, out, batch, single, [&](In v, In g, Out o, unsigned nm) {
      runs(stream, hipk::AdjointTerm<T>{adjDest, adjPartner, g, v}, o, nm);
    });
  } else {
    // both lists with the first product, whichever it is
    const RunLaunch<int32_t> byCol = runLaunch(d, m.cols, q, false), byRow = runLaunch(d, m.rows, q, false);
    const RunLaunch<int32_t>& runs = op == NormalEqJtVec ? byCol : byRow;
    if (runs.numRuns * q == 0) return;
    forOperandChunks<T>(h, values, x, out, batch, single, [&](In v, In xv, Out o, unsigned nm) {
      runs(stream, hipk::DotTerm<T>{runs.entry, runs.idx, v, xv}, o, nm);
    });
  }
}

// mv (a = values, b = x, out = A x) or outer (a = g, b = x, out = the gradient of the values) on `batch`
// members: one launch per chunk
template <typename T>
void hipBackendSymProduct(SymbolicCtx& sym, const SymProductMap& m, int32_t op, const T* const* a, const T* const* b,
                          T* const* out, int64_t q, int64_t batch, bool single) {
  using In = hipk::DataRef<const T>;
  using Out = hipk::DataRef<T>;
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  HipEntryMapDev& d = HipEntryMapDev::of(m.dev);
  if (op == SymProductMv) {
    const RunLaunch<int32_t> rows = runLaunch(d, m.rows, q, true);
    if (m.n * q == 0) return;
    forOperandChunks<T>(h, a, b, out, batch, single, [&](In v, In xv, Out o, unsigned nm) {
      rows(stream, hipk::DotTerm<T>{rows.entry, rows.idx, v, xv}, o, nm);
    });
  } else {
    const int32_t *entRow = d.get(m.entRow), *entCol = d.get(m.entCol);
    if (m.nnz == 0) return;
    const int64_t wgs = (m.nnz + hipk::kAsmThreads - 1) / hipk::kAsmThreads;
    forOperandChunks<T>(h, a, b, out, batch, single, [&](In g, In xv, Out o, unsigned nm) {
      hipk::symProductOuter<T><<<dim3((unsigned)wgs, nm), hipk::kAsmThreads, 0, stream>>>(m.nnz, (int32_t)q, entRow,
                                                                                          entCol, g, xv, o);
    });
  }
}

// ---- error bounds (hip_ordered_sum.h, hip_norm_est_kernels.h) ------------------
// r = b - A x and d = |A| |x| + |b| (b given), or d = |A| |x| alone (b, r NULL), on `batch` members: one
// launch per chunk over the row lists of mv
template <typename T>
void hipBackendSymResidual(SymbolicCtx& sym, const SymProductMap& m, const T* const* values, const T* const* x,
                           const T* const* b, T* const* r, T* const* d, int64_t q, int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  HipEntryMapDev& dv = HipEntryMapDev::of(m.dev);
  const RunLaunch<int32_t> rows = runLaunch(dv, m.rows, q, true);
  if (m.n * q == 0) return;
  const BatchPtrs<const T> vs = h.stage(values, batch, single), xs = h.stage(x, batch, single);
  const BatchPtrs<const T> bs = h.stage(b, batch, single);
  const BatchPtrs<T> rs = h.stage(r, batch, single), ds = h.stage(d, batch, single);
  const dim3 block(hipk::kAsmThreads);
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    const dim3 grid((unsigned)(rows.shortWgs + rows.longWgs), nm);
    if (b != nullptr) {
      hipk::symProductResidual<T, true><<<grid, block, 0, stream>>>(
          rows.numRuns, (int32_t)q, (int32_t)rows.shortWgs, rows.longWaves, rows.start, rows.longRuns, rows.entry,
          rows.idx, vs.at(q0), xs.at(q0), bs.at(q0), rs.at(q0), ds.at(q0));
    } else {
      hipk::symProductResidual<T, false><<<grid, block, 0, stream>>>(
          rows.numRuns, (int32_t)q, (int32_t)rows.shortWgs, rows.longWaves, rows.start, rows.longRuns, rows.entry,
          rows.idx, vs.at(q0), xs.at(q0), bs.at(q0), rs.at(q0), ds.at(q0));
    }
  });
}

// out[member q + j] = max over the n rows of ratio(|a[i, j]|, b[i, j]) (b given) or of a[i, j] (b NULL),
// in double: two launches per chunk, the partials of a chunk in ExtensionState::redPart
template <typename T>
void hipBackendColMax(SymbolicCtx& sym, const T* const* a, const T* const* b, int64_t n, int64_t q, double* out,
                      int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  const int64_t nParts = (n + hipk::kRedChunk - 1) / hipk::kRedChunk;
  BASPACHO_CHECK_LT(nParts * q, (int64_t)INT32_MAX);
  const int64_t chunk = std::min(batch, HipSymbolicCtx::kMaxGridY);
  hipk::RedPart* part = extState(h).reserveRedParts(chunk * q * nParts);
  const BatchPtrs<const T> as = h.stage(a, batch, single), bs = h.stage(b, batch, single);
  const double start = b != nullptr ? 0.0 : -std::numeric_limits<double>::infinity();
  h.forChunks(batch, chunk, [&](int64_t q0, unsigned nm) {
    if (nParts > 0) {
      const dim3 grid((unsigned)(nParts * q), nm);
      if (b != nullptr) {
        hipk::colMaxPartial<T, true><<<grid, hipk::kRedThreads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts,
                                                                             as.at(q0), bs.at(q0), part);
      } else {
        hipk::colMaxPartial<T, false><<<grid, hipk::kRedThreads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts,
                                                                              as.at(q0), bs.at(q0), part);
      }
    }
    hipk::colMaxFinal<<<dim3((unsigned)q, nm), hipk::kRedThreads, 0, stream>>>((int32_t)q, (int32_t)nParts, start,
                                                                             part, out + q0 * q);
  });
}

// one step of the 1-norm estimate (NormEstStep) on `batch` matrices whose work areas sit `stride` bytes
// apart from `work` on (normEstWorkBytes, hip_backend.h): one or two launches per chunk
template <typename T>
void hipBackendNormEstStep(SymbolicCtx& sym, int32_t step, void* work, const T* const* D, int64_t* state,
                           double* out, int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  const int64_t n = h.skel.order();
  const int64_t stride = normEstWorkBytes(n, sizeof(T)), partOff = normEstPartOffset(n, sizeof(T));
  const int64_t nParts = (n + hipk::kRedChunk - 1) / hipk::kRedChunk;
  const unsigned wgs = (unsigned)((n + hipk::kRedThreads - 1) / hipk::kRedThreads);
  BASPACHO_CHECK_LT(nParts, (int64_t)INT32_MAX);
  const BatchPtrs<const T> ds = h.stage(step == NormEstScale ? D : nullptr, batch, single);
  const int threads = hipk::kRedThreads;
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    const hipk::NormEstWork w{static_cast<char*>(work) + q0 * stride, stride, partOff};
    hipk::NormEstState* st = reinterpret_cast<hipk::NormEstState*>(state) + q0;
    const dim3 perElem(wgs, nm), perChunk((unsigned)nParts, nm), perMatrix(1, nm);
    switch (step) {
      case NormEstStart:
      case NormEstUnit:
      case NormEstAltVector:
        hipk::normEstWrite<T><<<perElem, threads, 0, stream>>>(n, step - NormEstStart, w, st);
        break;
      case NormEstScale:
        hipk::normEstScale<T><<<perElem, threads, 0, stream>>>(n, w, ds.at(q0));
        break;
      case NormEstSum:
        hipk::normEstSumPartial<T, true><<<perChunk, threads, 0, stream>>>(n, w);
        hipk::normEstSumFinal<<<perMatrix, threads, 0, stream>>>(n, (int32_t)nParts, false, w, st, out + q0);
        break;
      case NormEstAltSum:
        hipk::normEstSumPartial<T, false><<<perChunk, threads, 0, stream>>>(n, w);
        hipk::normEstSumFinal<<<perMatrix, threads, 0, stream>>>(n, (int32_t)nParts, true, w, st, out + q0);
        break;
      case NormEstArgMax:
        hipk::normEstArgMaxPartial<T><<<perChunk, threads, 0, stream>>>(n, w);
        hipk::normEstArgMaxFinal<T><<<perMatrix, threads, 0, stream>>>(n, (int32_t)nParts, w, st);
        break;
      default:
        throw std::runtime_error("invNorm1Estimate: unknown step " + std::to_string(step));
    }
  });
}

// ---- preconditioned conjugate gradient (hip_cg_kernels.h) ------------------------
// one piece of an iteration (CgOp) on `batch` matrices: one to four launches per chunk, nothing allocated
// but the tables of a preconditioner plan, which the first call that needs them uploads
static_assert(hipk::kCgMaxBlock == kCgMaxBlockWidth, "the build kernel's LDS holds the widest block of the plan");
static_assert(hipk::kCgFsaiMaxRow == kCgFsaiMaxRow, "the build kernel's LDS holds the widest row of the plan");
static_assert(hipk::kRedChunk == 1024, "chunkLongFirst of a CgFsaiPlan counts in chunks of 1024 scalars");
template <typename T>
void hipBackendCg(SymbolicCtx& sym, const CgArgs<T>& a, int64_t batch, bool single) {
  using In = hipk::DataRef<const T>;
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  const int64_t n = a.n, q = a.q;
  const int64_t nParts = (n + hipk::kRedChunk - 1) / hipk::kRedChunk;
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT(nParts * q, (int64_t)INT32_MAX);
  const int64_t perElemWgs = (n * q + hipk::kRedThreads - 1) / hipk::kRedThreads;
  BASPACHO_CHECK_LT(perElemWgs, (int64_t)INT32_MAX);
  const int64_t stride = cgWorkBytes(n, q), badOff = cgBadOffset(n, q);
  const bool builtIn = a.kind == CgJacobi || a.kind == CgBlockJacobi;
  hipk::CgPrecondDev pl{};
  int64_t numBlocks = 0;
  if ((a.op == CgPrecond || a.op == CgBuild) && builtIn) {
    const CgPrecondPlan& plan = cgPrecondPlan(*a.map, a.kind);
    HipEntryMapDev& d = HipEntryMapDev::of(a.map->dev);
    pl = {d.get(plan.blockStart), d.get(plan.blockOff),  d.get(plan.scalarBlock),
          d.get(plan.itemStart),  d.get(plan.itemEntry), d.get(plan.itemPos)};
    numBlocks = plan.numBlocks;
  }
  const bool fsai = a.kind == CgFsai && (a.op == CgBuild || a.op == CgFsaiApply);
  hipk::CgFsaiDev fs{};
  if (fsai) {
    const CgFsaiPlan& plan = cgFsaiPlan(*a.map);
    HipEntryMapDev& d = HipEntryMapDev::of(a.map->dev);
    fs = {d.get(plan.rowStart),      d.get(plan.cols),          d.get(plan.itemStart),        d.get(plan.itemEntry),
          d.get(plan.itemPos),       d.get(plan.colRuns.start), d.get(plan.colRuns.entry),    d.get(plan.colRuns.idx),
          d.get(plan.colRuns.longRuns), d.get(plan.chunkLongFirst)};
  }
  const BatchPtrs<const T> i0 = h.stage(a.in0, batch, single), i1 = h.stage(a.in1, batch, single);
  const BatchPtrs<T> o0 = h.stage(a.out0, batch, single), o1 = h.stage(a.out1, batch, single);
  const int threads = hipk::kRedThreads;
  const double tol2 = a.tol * a.tol;
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, badOff};
    hipk::CgState* st = reinterpret_cast<hipk::CgState*>(a.state) + q0 * q;
    const dim3 perChunk((unsigned)(nParts * q), nm), perColumn((unsigned)q, nm), perElem((unsigned)perElemWgs, nm);
    const In out1c{o1.at(q0).single, (const T* const*)o1.at(q0).many};
    const auto fold = [&](int32_t kind) {
      hipk::cgFold<<<perColumn, threads, 0, stream>>>((int32_t)q, (int32_t)nParts, kind, a.plain, tol2, a.maxSteps, w,
                                                     st);
    };
    const auto dot = [&](In x, In y, bool always) {
      if (nParts > 0) {
        hipk::cgDotPartial<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, x, y, w, st, always);
      }
    };
    switch (a.op) {
      case CgInit:
        dot(i0.at(q0), i0.at(q0), true);
        fold(hipk::CgFoldBB);
        if (perElemWgs > 0) hipk::cgStart<T><<<perElem, threads, 0, stream>>>(n, (int32_t)q, o0.at(q0), o1.at(q0), st);
        dot(out1c, out1c, false);
        fold(hipk::CgFoldRR0);
        break;
      case CgAlpha:
        dot(i0.at(q0), i1.at(q0), false);
        fold(hipk::CgFoldAlpha);
        break;
      case CgUpdate:
        if (nParts > 0) {
          hipk::cgUpdateXR<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, i0.at(q0), i1.at(q0),
                                                                o0.at(q0), o1.at(q0), w, st);
        }
        fold(hipk::CgFoldRR);
        break;
      case CgPrecond:
        if (nParts > 0) {
          if (a.kind == CgJacobi) {
            hipk::cgPrecond<T, 1><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, pl, i0.at(q0),
                                                                    i1.at(q0), o0.at(q0), w, st);
          } else if (a.kind == CgBlockJacobi) {
            hipk::cgPrecond<T, 2><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, pl, i0.at(q0),
                                                                    i1.at(q0), o0.at(q0), w, st);
          } else {
            hipk::cgPrecond<T, 0><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, pl, i0.at(q0),
                                                                    i1.at(q0), o0.at(q0), w, st);
          }
        }
        fold(hipk::CgFoldBeta);
        break;
      case CgDirection:
        if (perElemWgs > 0) {
          hipk::cgDirection<T><<<perElem, threads, 0, stream>>>(n, (int32_t)q, i0.at(q0), o0.at(q0), st);
        }
        break;
      case CgFsaiApply:
        if (perElemWgs > 0) {
          hipk::cgFsaiLower<T><<<perElem, threads, 0, stream>>>(n, (int32_t)q, fs, i0.at(q0), i1.at(q0), o1.at(q0), st);
          hipk::cgFsaiUpper<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, fs, i0.at(q0), out1c,
                                                                  i1.at(q0), o0.at(q0), w, st);
        }
        fold(hipk::CgFoldBeta);
        break;
      case CgBuild:
        if (fsai) {
          if (n > 0) {
            const int64_t wgs = (n + hipk::kCgFsaiRowsPerWg - 1) / hipk::kCgFsaiRowsPerWg;
            hipk::cgFsaiBuild<T><<<dim3((unsigned)wgs, nm), 64 * hipk::kCgFsaiRowsPerWg, 0, stream>>>(n, fs, i0.at(q0),
                                                                                                     o0.at(q0), w);
          }
          hipk::cgFsaiStatus<<<dim3(1, nm), threads, 0, stream>>>(n, fs, w, a.status + 2 * q0);
          break;
        }
        if (numBlocks > 0) {
          if (a.kind == CgJacobi) {
            hipk::cgJacobiBuild<T><<<dim3((unsigned)((n + threads - 1) / threads), nm), threads, 0, stream>>>(
                n, pl, i0.at(q0), o0.at(q0), w);
          } else {
            hipk::cgBlockBuild<T><<<dim3((unsigned)numBlocks, nm), hipk::kCgBuildThreads, 0, stream>>>(pl, i0.at(q0),
                                                                                                      o0.at(q0), w);
          }
        }
        hipk::cgPrecondStatus<<<dim3(1, nm), threads, 0, stream>>>(numBlocks, pl, w, a.status + 2 * q0);
        break;
      default:
        throw std::runtime_error("cg: unknown operation " + std::to_string(a.op));
    }
  });
}

// ---- matrix-free least squares (hip_cgls_kernels.h) ------------------------------
// one piece of CGLS (CglsOp) on `batch` Jacobians: one to three launches per chunk, nothing allocated but
// the tables of the map, each uploaded by the first call that needs it
template <typename T>
void hipBackendCgls(SymbolicCtx& sym, const CglsArgs<T>& a, int64_t batch, bool single) {
  using In = hipk::DataRef<const T>;
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  const JacobianProductMap& map = *a.map;
  const int64_t m = map.m, n = map.n, q = a.q;
  const int64_t nParts = (n + hipk::kRedChunk - 1) / hipk::kRedChunk, mParts = (m + hipk::kRedChunk - 1) / hipk::kRedChunk;
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT((nParts + mParts) * q, (int64_t)INT32_MAX);
  const int64_t stride = cglsWorkBytes(m, n, q), badOff = cglsBadOffset(m, n, q);
  HipEntryMapDev& d = HipEntryMapDev::of(map.dev);
  const auto runsOf = [&](const RunList& r, int64_t vectors) {
    const RunLaunch<int32_t> l = runLaunch(d, r, vectors, true);
    return hipk::CglsRuns{l.numRuns, l.longWaves, (int32_t)l.shortWgs, l.start, l.longRuns, l.entry, l.idx};
  };
  const auto gridOf = [](const hipk::CglsRuns& r, unsigned nm) {
    const int64_t longWgs = (r.numLongWaves + hipk::kAsmWavesPerWg - 1) / hipk::kAsmWavesPerWg;
    return dim3((unsigned)(r.shortWgs + longWgs), nm);
  };
  hipk::CglsRuns runs{};
  if (a.op == CglsJv || a.op == CglsJtv) runs = runsOf(a.op == CglsJv ? map.rows : map.cols, q);
  if (a.op == CglsColSq) runs = runsOf(map.cols, 1);
  hipk::CglsRuns rowRuns{}, colRuns{};
  if (a.op == CglsIterate) {
    rowRuns = runsOf(map.rows, q);
    colRuns = runsOf(map.cols, q);
  }
  hipk::CgPrecondDev pl{};
  hipk::CglsBlockItems items{};
  int64_t numBlocks = a.op == CglsBuild ? n : 0;
  if ((a.op == CglsApply || a.op == CglsBuild || a.op == CglsIterate) && a.kind == CgBlockJacobi) {
    const JacBlockPlan& plan = jacBlockPlan(map);
    pl = {d.get(plan.blockStart), d.get(plan.blockOff), d.get(plan.scalarBlock), nullptr, nullptr, nullptr};
    if (a.op == CglsBuild) items = {d.get(plan.itemStart), d.get(plan.itemA), d.get(plan.itemB), d.get(plan.itemPos)};
    numBlocks = plan.numBlocks;
  } else if (a.op == CglsBuild) {
    pl.blockStart = d.get(map.scalarStart);
  }
  const BatchPtrs<const T> vs = h.stage(a.values, batch, single), ws = h.stage(a.vec, batch, single);
  const BatchPtrs<const T> as = h.stage(a.addend, batch, single), ds = h.stage(a.damp, batch, single);
  const BatchPtrs<T> xs = h.stage(a.x, batch, single), os = h.stage(a.out, batch, single);
  const BatchPtrs<double> cs = h.stage(a.colsq, batch, single);
  const BatchPtrs<T> ps = h.stage(a.p, batch, single), ts = h.stage(a.t, batch, single);
  const BatchPtrs<T> rs = h.stage(a.res, batch, single), ss = h.stage(a.s, batch, single);
  const BatchPtrs<T> zs = h.stage(a.z, batch, single);
  const BatchPtrs<const T> ms = h.stage(a.minv, batch, single);
  const int threads = hipk::kRedThreads;
  const double tol2 = a.tol * a.tol;
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, badOff};
    hipk::CgState* st = a.state ? reinterpret_cast<hipk::CgState*>(a.state) + q0 * q : nullptr;
    const In xIn{xs.at(q0).single, (const T* const*)xs.at(q0).many};
    const hipk::DataRef<const double> cIn{cs.at(q0).single, (const double* const*)cs.at(q0).many};
    const dim3 perColumn((unsigned)q, nm), nChunks((unsigned)(nParts * q), nm), mChunks((unsigned)(mParts * q), nm);
    const dim3 perScalar((unsigned)((n + threads - 1) / threads), nm);
    const auto asIn = [](const hipk::DataRef<T>& r) { return In{r.single, (const T* const*)r.many}; };
    // delta = |t|^2 + p^T D p: the partials of t.t, then (d given) those of (p p) d, one fold
    const auto delta = [&](In t, In p, In d, bool damped, bool fold) {
      const int64_t total = mParts + (damped ? nParts : 0);
      const int64_t chunks = mParts + (damped ? nParts : 0);
      if (chunks > 0) {
        hipk::cglsDeltaPartial<T><<<dim3((unsigned)(chunks * q), nm), threads, 0, stream>>>(
            m, n, (int32_t)q, (int32_t)mParts, (int32_t)total, t, p, d, w, st);
      }
      if (fold) {
        hipk::cgFold<<<perColumn, threads, 0, stream>>>((int32_t)q, (int32_t)total, hipk::CgFoldAlpha, false, 0.0, 0, w,
                                                       st);
      }
      return total;
    };
    const auto update = [&](In p, In t, hipk::DataRef<T> x, hipk::DataRef<T> res) {
      if (nParts + mParts > 0) {
        hipk::cglsUpdate<T><<<dim3((unsigned)((nParts + mParts) * q), nm), threads, 0, stream>>>(
            n, m, (int32_t)q, (int32_t)nParts, p, t, x, res, st);
      }
    };
    const auto apply = [&](In minv, In sv, hipk::DataRef<T> z, bool start) {
      if (nParts > 0) {
        if (a.kind == CgJacobi) {
          hipk::cglsApply<T, 1><<<nChunks, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, pl, minv, sv, z, w, st);
        } else if (a.kind == CgBlockJacobi) {
          hipk::cglsApply<T, 2><<<nChunks, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, pl, minv, sv, z, w, st);
        } else {
          hipk::cglsApply<T, 0><<<nChunks, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, pl, minv, sv, z, w, st);
        }
      }
      hipk::cglsFold<<<perColumn, threads, 0, stream>>>((int32_t)q, (int32_t)nParts, start, w, st);
    };
    switch (a.op) {
      case CglsJv:
      case CglsJtv: {
        if (runs.numRuns * q == 0) break;
        const dim3 grid = gridOf(runs, nm);
        const auto launch = [&](auto epi) {
          hipk::cglsProduct<T, decltype(epi)::value><<<grid, hipk::kAsmThreads, 0, stream>>>(
              runs, (int32_t)q, vs.at(q0), ws.at(q0), as.at(q0), ds.at(q0), xIn, os.at(q0), st);
        };
        if (a.epi == hipk::CglsResidual) {
          launch(std::integral_constant<int, hipk::CglsResidual>());
        } else if (a.epi == hipk::CglsNormal) {
          launch(std::integral_constant<int, hipk::CglsNormal>());
        } else {
          launch(std::integral_constant<int, hipk::CglsPlain>());
        }
        break;
      }
      case CglsColSq:
        if (n > 0) hipk::cglsColSq<T><<<gridOf(runs, nm), hipk::kAsmThreads, 0, stream>>>(runs, vs.at(q0), cs.at(q0));
        break;
      case CglsDamp:
        if (n > 0) hipk::cglsDamp<T><<<perScalar, threads, 0, stream>>>(n, a.alpha, a.beta, cIn, os.at(q0));
        break;
      case CglsInit:
        if (nParts > 0) {
          hipk::cgDotPartial<T><<<nChunks, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, ws.at(q0), ws.at(q0), w,
                                                                 st, true);
        }
        hipk::cgFold<<<perColumn, threads, 0, stream>>>((int32_t)q, (int32_t)nParts, hipk::CgFoldBB, false, tol2,
                                                       a.maxSteps, w, st);
        if (n > 0) {
          hipk::cgStart<T><<<dim3((unsigned)((n * q + threads - 1) / threads), nm), threads, 0, stream>>>(
              n, (int32_t)q, xs.at(q0), xs.at(q0), st);
        }
        break;
      case CglsDelta:
        delta(ws.at(q0), xIn, ds.at(q0), a.damp != nullptr, true);
        break;
      case CglsUpdate:
        update(ws.at(q0), as.at(q0), xs.at(q0), os.at(q0));
        break;
      case CglsApply:
        apply(ds.at(q0), ws.at(q0), os.at(q0), a.start);
        break;
      case CglsIterate: {
        const In pIn = asIn(ps.at(q0)), tIn = asIn(ts.at(q0)), sIn = asIn(ss.at(q0));
        if (a.phase != 2) {
          if (rowRuns.numRuns * q > 0) {
            hipk::cglsProduct<T, hipk::CglsPlain><<<gridOf(rowRuns, nm), hipk::kAsmThreads, 0, stream>>>(
                rowRuns, (int32_t)q, vs.at(q0), pIn, In{}, In{}, In{}, ts.at(q0), nullptr);
          }
          // the fold of delta rides in the update's launch: the same sum, the same decision
          const int64_t total = delta(tIn, pIn, ds.at(q0), a.damp != nullptr, false);
          if (nParts + mParts > 0) {
            hipk::cglsAlphaUpdate<T><<<dim3((unsigned)((nParts + mParts) * q), nm), threads, 0, stream>>>(
                n, m, (int32_t)q, (int32_t)nParts, (int32_t)total, pIn, tIn, xs.at(q0), rs.at(q0), w, st);
          }
          if (colRuns.numRuns * q > 0) {
            hipk::cglsProduct<T, hipk::CglsNormal><<<gridOf(colRuns, nm), hipk::kAsmThreads, 0, stream>>>(
                colRuns, (int32_t)q, vs.at(q0), asIn(rs.at(q0)), as.at(q0), ds.at(q0),
                a.damp != nullptr ? xIn : In{}, ss.at(q0), st);
          }
        }
        if (a.phase != 1) {
          apply(ms.at(q0), sIn, zs.at(q0), false);
          const int64_t wgs = (n * q + threads - 1) / threads;
          if (wgs > 0) {
            hipk::cgDirection<T><<<dim3((unsigned)wgs, nm), threads, 0, stream>>>(n, (int32_t)q, asIn(zs.at(q0)),
                                                                                  ps.at(q0), st);
          }
        }
        break;
      }
      case CglsBuild:
        if (numBlocks > 0) {
          if (a.kind == CgJacobi) {
            hipk::cglsJacobiBuild<T><<<perScalar, threads, 0, stream>>>(n, cIn, ds.at(q0), os.at(q0), w);
          } else {
            hipk::cglsBlockBuild<T><<<dim3((unsigned)numBlocks, nm), hipk::kCgBuildThreads, 0, stream>>>(
                pl, items, vs.at(q0), ds.at(q0), os.at(q0), w);
          }
        }
        hipk::cgPrecondStatus<<<dim3(1, nm), threads, 0, stream>>>(numBlocks, pl, w, a.status + 2 * q0);
        break;
      default:
        throw std::runtime_error("cgls: unknown operation " + std::to_string(a.op));
    }
  });
}

// ---- implicit Schur elimination (hip_schur_kernels.h) ----------------------------
// one piece (SchurOp) on `batch` Jacobians: one or two launches per chunk, nothing allocated but the tables
// of the map, each uploaded by the first call that needs it
static_assert(hipk::kSchurMaxW == kSchurMaxElimWidth, "the group kernel's registers hold the widest eliminated param");
template <typename T>
void hipBackendJacSchur(SymbolicCtx& sym, const JacSchurArgs<T>& a, int64_t batch, bool single) {
  using In = hipk::DataRef<const T>;
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  const JacSchurMap& map = *a.map;
  const int64_t m = map.m, n = map.n, q = a.q;
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  HipEntryMapDev& d = HipEntryMapDev::of(map.dev);
  const JacBlockPlan& plan = *map.elimBlocks;
  const BatchPtrs<const T> vs = h.stage(a.values, batch, single), ds = h.stage(a.damp, batch, single);
  const BatchPtrs<const T> bs = h.stage(a.binv, batch, single), ws = h.stage(a.vec, batch, single);
  const BatchPtrs<const T> gs = h.stage(a.full, batch, single);
  const BatchPtrs<T> ts = h.stage(a.t, batch, single), os = h.stage(a.out, batch, single);
  if (a.op == SchurBuild) {
    const int64_t stride = cglsWorkBytes(m, n, 1), badOff = cglsBadOffset(m, n, 1);
    const hipk::CgPrecondDev pl{d.get(plan.blockStart), d.get(plan.blockOff), d.get(plan.scalarBlock), nullptr, nullptr,
                                nullptr};
    const hipk::CglsBlockItems items{d.get(plan.itemStart), d.get(plan.itemA), d.get(plan.itemB), d.get(plan.itemPos),
                                     d.get(plan.blockWidth)};
    // (the output of the build is a.out: the inverses)
    h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
      const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, badOff};
      hipk::cglsBlockBuild<T><<<dim3((unsigned)plan.numBlocks, nm), hipk::kCgBuildThreads, 0, stream>>>(
          pl, items, vs.at(q0), ds.at(q0), os.at(q0), w);
      hipk::cgPrecondStatus<<<dim3(1, nm), hipk::kRedThreads, 0, stream>>>(plan.numBlocks, pl, w, a.status + 2 * q0);
    });
    return;
  }
  if (a.op == SchurPrecondBuild) {
    const int64_t stride = cglsWorkBytes(m, n, 1), badOff = cglsBadOffset(m, n, 1);
    const BatchPtrs<const double> cs = h.stage(a.colsq, batch, single);
    const int32_t* keptScalar = d.get(map.keptScalar);
    hipk::CgPrecondDev pl{keptScalar, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipk::CglsBlockItems items{};
    int64_t numBlocks = map.nK;
    if (a.kind == CgBlockJacobi) {
      const JacBlockPlan& kp = jacSchurKeptPlan(map);
      pl = {d.get(kp.blockStart), d.get(kp.blockOff), d.get(kp.scalarBlock), nullptr, nullptr, nullptr};
      items = {d.get(kp.itemStart), d.get(kp.itemA), d.get(kp.itemB), d.get(kp.itemPos), d.get(kp.blockWidth)};
      numBlocks = kp.numBlocks;
    }
    h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
      const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, badOff};
      if (a.kind == CgBlockJacobi) {
        hipk::cglsBlockBuild<T><<<dim3((unsigned)numBlocks, nm), hipk::kCgBuildThreads, 0, stream>>>(
            pl, items, vs.at(q0), ds.at(q0), os.at(q0), w);
      } else {
        const unsigned wgs = (unsigned)((map.nK + hipk::kRedThreads - 1) / hipk::kRedThreads);
        hipk::schurJacobiBuild<T><<<dim3(wgs, nm), hipk::kRedThreads, 0, stream>>>(map.nK, keptScalar, cs.at(q0),
                                                                                  ds.at(q0), os.at(q0), w);
      }
      hipk::cgPrecondStatus<<<dim3(1, nm), hipk::kRedThreads, 0, stream>>>(numBlocks, pl, w, a.status + 2 * q0);
    });
    return;
  }
  if (a.op == SchurPrecondApply) {
    const int64_t nK = map.nK, nParts = (nK + hipk::kRedChunk - 1) / hipk::kRedChunk;
    BASPACHO_CHECK_LT(nParts * q, (int64_t)INT32_MAX);
    const int64_t stride = cgWorkBytes(nK, q), badOff = cgBadOffset(nK, q);
    hipk::CgPrecondDev pl{};
    if (a.kind == CgBlockJacobi) {
      const JacBlockPlan& kp = jacSchurKeptPlan(map);
      pl = {d.get(map.keptBlockStart), d.get(kp.blockOff), d.get(map.keptScalarBlock), nullptr, nullptr, nullptr};
    }
    h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
      const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, badOff};
      hipk::CgState* st = reinterpret_cast<hipk::CgState*>(a.state) + q0 * q;
      const dim3 perChunk((unsigned)(nParts * q), nm);
      if (a.kind == CgBlockJacobi) {
        hipk::cgPrecond<T, 2><<<perChunk, hipk::kRedThreads, 0, stream>>>(nK, (int32_t)q, (int32_t)nParts, pl, bs.at(q0),
                                                                         ws.at(q0), os.at(q0), w, st);
      } else {
        hipk::cgPrecond<T, 1><<<perChunk, hipk::kRedThreads, 0, stream>>>(nK, (int32_t)q, (int32_t)nParts, pl, bs.at(q0),
                                                                         ws.at(q0), os.at(q0), w, st);
      }
      hipk::cgFold<<<dim3((unsigned)q, nm), hipk::kRedThreads, 0, stream>>>((int32_t)q, (int32_t)nParts, hipk::CgFoldBeta,
                                                                          false, 0.0, 0, w, st);
    });
    return;
  }
  if (a.op == SchurSJacobiBuild) {  // the block diagonal of S: the chunks, then the blocks
    const JacSchurJacobiPlan& sp = jacSchurJacobiPlan(map);
    const int64_t stride = cglsWorkBytes(m, n, 1), badOff = cglsBadOffset(m, n, 1);
    const BatchPtrs<double> ps = h.stage(a.partials, batch, single);
    const hipk::SchurJacobiDev sj{d.get(sp.chunkPair),   d.get(sp.chunkBlock), d.get(sp.chunkPart), d.get(sp.pairElim),
                                  d.get(sp.pairRow),     d.get(sp.pairRec),    d.get(sp.rec),       d.get(map.keptWidth),
                                  d.get(map.keptFirst),  d.get(map.elimOff),   d.get(sp.blockChunk), d.get(plan.blockOff),
                                  d.get(sp.blockOff)};
    const hipk::CgPrecondDev pl{sj.keptFirst, sj.blockOff, nullptr, nullptr, nullptr, nullptr};
    const int64_t numChunks = sp.numChunks(), numBlocks = sp.numBlocks;
    BASPACHO_CHECK_LT(numChunks, (int64_t)INT32_MAX);
    h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
      const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, badOff};
      const hipk::DataRef<double> pOut = ps.at(q0);
      if (numChunks > 0) {
        hipk::schurJacobiChunks<T><<<dim3((unsigned)numChunks, nm), hipk::kSjThreads, 0, stream>>>(sj, vs.at(q0),
                                                                                                 bs.at(q0), pOut);
      }
      if (numBlocks > 0) {
        hipk::schurJacobiBlocks<T><<<dim3((unsigned)numBlocks, nm), hipk::kCgBuildThreads, 0, stream>>>(
            sj, hipk::DataRef<const double>{pOut.single, (const double* const*)pOut.many}, ds.at(q0), os.at(q0), w);
      }
      hipk::cgPrecondStatus<<<dim3(1, nm), hipk::kRedThreads, 0, stream>>>(numBlocks, pl, w, a.status + 2 * q0);
    });
    return;
  }
  if (a.op == SchurSJacobiApply) {  // SchurPrecondApply of kind 2 on the new plan's block offsets
    const JacSchurJacobiPlan& sp = jacSchurJacobiPlan(map);
    const int64_t nK = map.nK, nParts = (nK + hipk::kRedChunk - 1) / hipk::kRedChunk;
    BASPACHO_CHECK_LT(nParts * q, (int64_t)INT32_MAX);
    const int64_t stride = cgWorkBytes(nK, q), badOff = cgBadOffset(nK, q);
    const hipk::CgPrecondDev pl{d.get(map.keptBlockStart), d.get(sp.blockOff), d.get(map.keptScalarBlock), nullptr,
                                nullptr, nullptr};
    h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
      const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, badOff};
      hipk::CgState* st = reinterpret_cast<hipk::CgState*>(a.state) + q0 * q;
      hipk::cgPrecond<T, 2><<<dim3((unsigned)(nParts * q), nm), hipk::kRedThreads, 0, stream>>>(
          nK, (int32_t)q, (int32_t)nParts, pl, bs.at(q0), ws.at(q0), os.at(q0), w, st);
      hipk::cgFold<<<dim3((unsigned)q, nm), hipk::kRedThreads, 0, stream>>>((int32_t)q, (int32_t)nParts, hipk::CgFoldBeta,
                                                                          false, 0.0, 0, w, st);
    });
    return;
  }
  const hipk::SchurDev sd{map.numElim,
                          (int64_t)map.freeRows.size(),
                          map.nK,
                          d.get(map.groupStart),
                          d.get(map.groupRow),
                          d.get(map.freeRows),
                          d.get(map.elimOff),
                          d.get(map.elimScalar),
                          d.get(map.keptScalar),
                          d.get(plan.blockOff),
                          d.get(map.rowsKept.start),
                          d.get(map.rowsKept.entry),
                          d.get(map.rowsKept.idx),
                          d.get(map.rowsElim.start),
                          d.get(map.rowsElim.entry),
                          d.get(map.rowsElim.idx),
                          d.get(map.colsElim.start),
                          d.get(map.colsElim.entry),
                          d.get(map.colsElim.idx)};
  const int64_t units = map.numElim + (int64_t)map.freeRows.size() + (a.op == SchurBack ? map.nK : 0);
  const int64_t groupWgs = (units * q + hipk::kAsmThreads - 1) / hipk::kAsmThreads;
  BASPACHO_CHECK_LT(groupWgs, (int64_t)INT32_MAX);
  const RunLaunch<int32_t> l = runLaunch(d, map.colsKept, q, true);
  const hipk::CglsRuns cols{l.numRuns, l.longWaves, (int32_t)l.shortWgs, l.start, l.longRuns, l.entry, l.idx};
  const int32_t* keptScalar = d.get(map.keptScalar);
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    const hipk::CgState* st = a.state ? reinterpret_cast<const hipk::CgState*>(a.state) + q0 * q : nullptr;
    const dim3 groupGrid((unsigned)groupWgs, nm), colGrid((unsigned)(l.shortWgs + l.longWgs), nm);
    const In tIn{ts.at(q0).single, (const T* const*)ts.at(q0).many};
    switch (a.op) {
      case SchurMv:
        hipk::schurGroups<T, hipk::SchurProduct><<<groupGrid, hipk::kAsmThreads, 0, stream>>>(
            sd, (int32_t)q, vs.at(q0), bs.at(q0), ws.at(q0), In{}, ts.at(q0), os.at(q0), st);
        hipk::schurKeptColumns<T, hipk::SchurProduct><<<colGrid, hipk::kAsmThreads, 0, stream>>>(
            cols, keptScalar, (int32_t)q, vs.at(q0), tIn, ds.at(q0), ws.at(q0), os.at(q0), st);
        break;
      case SchurReduce:
        hipk::schurGroups<T, hipk::SchurReduce><<<groupGrid, hipk::kAsmThreads, 0, stream>>>(
            sd, (int32_t)q, vs.at(q0), bs.at(q0), In{}, gs.at(q0), ts.at(q0), os.at(q0), nullptr);
        hipk::schurKeptColumns<T, hipk::SchurReduce><<<colGrid, hipk::kAsmThreads, 0, stream>>>(
            cols, keptScalar, (int32_t)q, vs.at(q0), tIn, In{}, gs.at(q0), os.at(q0), nullptr);
        break;
      case SchurBack:
        hipk::schurGroups<T, hipk::SchurBack><<<groupGrid, hipk::kAsmThreads, 0, stream>>>(
            sd, (int32_t)q, vs.at(q0), bs.at(q0), ws.at(q0), gs.at(q0), ts.at(q0), os.at(q0), nullptr);
        break;
      default:
        throw std::runtime_error("jacobian schur: unknown operation " + std::to_string(a.op));
    }
  });
}

// ---- the Lanczos recurrence (hip_lanczos_kernels.h) ------------------------------
// one piece of a step (LanczosOp) on `batch` matrices: one to three launches per chunk, nothing allocated
template <typename T>
void hipBackendLanczos(SymbolicCtx& sym, const LanczosArgs<T>& a, int64_t batch, bool single) {
  using In = hipk::DataRef<const T>;
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  const int64_t n = a.n, q = a.q, kmax = a.kmax;
  const int64_t nParts = (n + hipk::kRedChunk - 1) / hipk::kRedChunk;
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT(nParts * q, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT(kmax * q, (int64_t)INT32_MAX);
  const int64_t perElemWgs = (n * q + hipk::kRedThreads - 1) / hipk::kRedThreads;
  BASPACHO_CHECK_LT(perElemWgs, (int64_t)INT32_MAX);
  const int64_t stride = lanczosWorkBytes(n, q, kmax), projOff = lanczosProjOffset(n, q, kmax);
  const BatchPtrs<T> vec = h.stage(a.vec, batch, single), basis = h.stage(a.basis, batch, single);
  const int threads = hipk::kRedThreads;
  const double thr2 = a.breakdown * a.breakdown;
  const int64_t slotOff = a.slot * a.slotStride, prevOff = a.prev * a.slotStride;
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    const hipk::CgWork w{static_cast<char*>(a.work) + q0 * stride, stride, projOff};
    hipk::LzState* st = reinterpret_cast<hipk::LzState*>(a.state) + q0 * q;
    double* coef = a.coef ? a.coef + q0 * q * 2 * kmax : nullptr;
    const dim3 perChunk((unsigned)(nParts * q), nm), perColumn((unsigned)q, nm), perElem((unsigned)perElemWgs, nm);
    const In vecIn{vec.at(q0).single, (const T* const*)vec.at(q0).many};
    const In basisIn{basis.at(q0).single, (const T* const*)basis.at(q0).many};
    const auto fold = [&](int32_t kind) {
      hipk::lzFold<<<perColumn, threads, 0, stream>>>((int32_t)q, (int32_t)nParts, kind, thr2, kmax, w, st, coef);
    };
    switch (a.op) {
      case LzInit:
        if (nParts > 0) {
          hipk::cgDotPartial<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, vecIn, vecIn, w,
                                                                  nullptr, true);  // (always: no record is read)
        }
        fold(hipk::LzFoldVV);
        if (perElemWgs > 0) {
          hipk::lzNormalize<T><<<perElem, threads, 0, stream>>>(n, (int32_t)q, true, vecIn, basis.at(q0), slotOff, st);
        }
        break;
      case LzAlpha:
        if (nParts > 0) {
          hipk::lzDotPartial<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, basisIn, slotOff,
                                                                  vecIn, w, st);
        }
        fold(hipk::LzFoldAlpha);
        break;
      case LzUpdate:
        if (nParts > 0) {
          hipk::lzUpdate<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, basisIn, slotOff, prevOff,
                                                              vec.at(q0), w, st);
        }
        if (a.fold) fold(hipk::LzFoldStep);
        break;
      case LzProject:
        if (nParts > 0) {
          hipk::lzProjectPartial<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, (int32_t)a.count,
                                                                      basisIn, a.slotStride, vecIn, w, st);
        }
        hipk::lzProjectFold<<<dim3((unsigned)(a.count * q), nm), threads, 0, stream>>>((int32_t)q, (int32_t)nParts,
                                                                                        kmax, w, st);
        break;
      case LzSubtract:
        if (nParts > 0) {
          hipk::lzSubtract<T><<<perChunk, threads, 0, stream>>>(n, (int32_t)q, (int32_t)nParts, (int32_t)a.count, kmax,
                                                                basisIn, a.slotStride, vec.at(q0), w, st);
        }
        if (a.fold) fold(hipk::LzFoldStep);
        break;
      case LzNormalize:
        if (perElemWgs > 0) {
          hipk::lzNormalize<T><<<perElem, threads, 0, stream>>>(n, (int32_t)q, false, vecIn, basis.at(q0), slotOff, st);
        }
        break;
      default:
        throw std::runtime_error("lanczos: unknown operation " + std::to_string(a.op));
    }
  });
}

// ---- combinations of basis vectors (kvCombine) -----------------------------------
// one launch per chunk of members: a workgroup per (1024-row chunk, column), the members on gridDim.y
template <typename T>
void hipBackendKrylovCombine(SymbolicCtx& sym, const KrylovCombineArgs<T>& a, int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  const int64_t n = a.n, q = a.q;
  const int64_t nParts = (n + hipk::kRedChunk - 1) / hipk::kRedChunk;
  if (nParts == 0) return;
  BASPACHO_CHECK_LT(q, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT(nParts * q, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT(a.count, (int64_t)INT32_MAX);
  const BatchPtrs<const T> basis = h.stage(a.basis, batch, single);
  const BatchPtrs<T> out = h.stage(a.out, batch, single);
  const int threads = hipk::kRedThreads;
  const int64_t slotOff = a.slot * a.slotStride;
  h.forChunks(batch, HipSymbolicCtx::kMaxGridY, [&](int64_t q0, unsigned nm) {
    const dim3 grid((unsigned)(nParts * q), nm);
    const double* y = a.y + q0 * q * a.nf * a.ldy;
    const int64_t* limit = a.limit + q0 * q;
    const auto launch = [&](auto nf) {
      hipk::kvCombine<T, decltype(nf)::value><<<grid, threads, 0, stream>>>(
          n, (int32_t)q, (int32_t)a.count, a.first, basis.at(q0), slotOff, a.slotStride, y, a.ldy, limit, out.at(q0),
          a.outStride, a.accumulate);
    };
    switch (a.nf) {
      case 1:
        launch(std::integral_constant<int, 1>());
        break;
      case 2:
        launch(std::integral_constant<int, 2>());
        break;
      case 3:
        launch(std::integral_constant<int, 3>());
        break;
      case 4:
        launch(std::integral_constant<int, 4>());
        break;
      default:
        throw std::runtime_error("krylovCombine: nf = " + std::to_string(a.nf) + " is outside [1, 4]");
    }
  });
}

// ---- reach solves (hip_reach_kernels.h) ---------------------------------------
// W (numCols x order, column-major) <- the unit columns of the plan's queries, solved through the lumps
// of their reach below the cut: one memset, the unit entries of the queries behind the cut, one launch
// of a workgroup per column group.  The caller runs solveLFrom(cutSpan) on W afterwards.
template <typename T>
void hipBackendReachSolveL(SymbolicCtx& sym, const ReachPlan& p, const T* L, T* W) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  const int64_t order = h.skel.order();
  if (p.numCols == 0 || order == 0) return;
  ReachDev& r = extState(h).reach;
  const hipk::SkelDev sk = h.skelDev();
  TableBlob blob;
  const size_t oGroups = blob.add(p.groups), oLumps = blob.add(p.reachLumps);
  const size_t oCol = blob.add(p.unitCol), oRow = blob.add(p.unitRow);
  // room for the tables of hipBackendGramBlocks too: the ring does not grow in the middle of a call
  const size_t gramBytes =
      TableBlob::sizeWith(TableBlob::sizeWith(TableBlob::sizeWith(0, p.items), p.rangeStart), p.rangePrefix);
  r.ring.reserve(std::max(blob.bytes.size(), gramBytes));
  hipCHECK(hipMemsetAsync(W, 0, (size_t)p.numCols * order * sizeof(T), stream));
  if (blob.bytes.empty()) return;
  const char* d = reinterpret_cast<const char*>(r.ring.push(blob.bytes.data(), blob.bytes.size(), stream));
  const int64_t nUnits = (int64_t)p.unitCol.size();
  if (nUnits > 0) {
    hipk::reachUnits<T><<<dim3((unsigned)((nUnits + 255) / 256)), 256, 0, stream>>>(
        reinterpret_cast<const int64_t*>(d + oCol), reinterpret_cast<const int64_t*>(d + oRow), nUnits, W, order);
  }
  if (!p.groups.empty()) {
    hipk::reachSolveL<T><<<dim3((unsigned)p.groups.size()), 256, 0, stream>>>(
        reinterpret_cast<const ReachGroup*>(d + oGroups), reinterpret_cast<const int32_t*>(d + oLumps), sk,
        hipk::DataRef<const T>{L, nullptr}, W, order);
  }
  hipCHECK(hipGetLastError());
}

// out[item.outOff ..] = W_P^T W_Q for every item of the plan: one launch of a workgroup per item
template <typename T>
void hipBackendGramBlocks(SymbolicCtx& sym, const ReachPlan& p, const T* W, T* out) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  if (p.items.empty()) return;
  ReachDev& r = extState(h).reach;
  TableBlob blob;
  const size_t oItems = blob.add(p.items), oStart = blob.add(p.rangeStart), oPrefix = blob.add(p.rangePrefix);
  const char* d = reinterpret_cast<const char*>(r.ring.push(blob.bytes.data(), blob.bytes.size(), stream));
  hipk::gramBlocks<T><<<dim3((unsigned)p.items.size()), 256, 0, stream>>>(
      reinterpret_cast<const GramItem*>(d + oItems), reinterpret_cast<const int64_t*>(d + oStart),
      reinterpret_cast<const int64_t*>(d + oPrefix), W, h.skel.order(), out);
  hipCHECK(hipGetLastError());
}

// the W workspace of inverseBlocks, kept with the extension state: room for `elems` values of T
template <typename T>
T* hipBackendReachWorkspace(SymbolicCtx& sym, int64_t elems) {
  HipSymbolicCtx& h = hipCtx(sym);
  h.checkDevice();
  return reinterpret_cast<T*>(extState(h).reach.reserve((size_t)std::max<int64_t>(elems, 1) * sizeof(T)));
}

// ---- products with the factor (hip_factor_product.h) ---------------------------
// y[q] = L[q] x[q] (transposed: L[q]^T x[q]) for `batch` members.  The plan is built and uploaded by the
// first product, whichever it is.  A chunk is one launch (two when y = L x has huge spans or y = L^T x
// has split strips), members on
// gridDim.y and groups of right-hand sides on gridDim.z; chunks are bounded by the partial sums they need
template <typename T>
void hipBackendFactorProduct(SymbolicCtx& sym, const T* const* L, bool transposed, const T* const* x, int64_t ldx,
                             T* const* y, int64_t ldy, int nRHS, int64_t batch, bool single) {
  HipSymbolicCtx& h = hipCtx(sym);
  const hipStream_t stream = h.stream;
  h.checkDevice();
  ExtensionState& ext = extState(h);
  if (!ext.factorProduct) {
    std::unique_ptr<FactorProductState> p(new FactorProductState);
    p->build(h.skel);
    ext.factorProduct = std::move(p);
  }
  FactorProductState& st = *ext.factorProduct;
  const int64_t order = h.skel.order();
  if (order == 0) return;
  BASPACHO_CHECK_LE(nRHS, 65535);
  const hipk::SkelDev sk = h.skelDev();
  const hipk::FactorProductDev pl = st.dev();
  const unsigned zGroups = (unsigned)((nRHS + hipk::kFpRhs - 1) / hipk::kFpRhs);
  // members per chunk: at most 256 MB of partial sums (fp64), at least one member
  int64_t chunk = std::min(batch, HipSymbolicCtx::kMaxGridY);
  if (transposed && st.host.partElems > 0) {
    const int64_t perMember = st.host.partElems * nRHS * (int64_t)sizeof(double);
    chunk = std::max<int64_t>(1, std::min(chunk, ((int64_t)256 << 20) / perMember));
    st.reservePart(chunk * nRHS);
  }
  const BatchPtrs<const T> ls = h.stage(L, batch, single), xs = h.stage(x, batch, single);
  const BatchPtrs<T> ys = h.stage(y, batch, single);
  const int64_t shortWgs = (order + hipk::kFpThreads - 1) / hipk::kFpThreads;
  const int64_t numLong = (int64_t)st.host.longRows.size();
  const int64_t longWgs = (numLong + hipk::kFpWaves - 1) / hipk::kFpWaves;
  const int64_t numTasks = (int64_t)st.host.ltTasks.size(), numSmall = (int64_t)st.host.smallCol.size();
  const int64_t smallWgs = (numSmall + hipk::kFpThreads - 1) / hipk::kFpThreads;
  const int64_t numFolds = (int64_t)st.host.ltFolds.size(), numHuge = (int64_t)st.host.hugeSpans.size();
  BASPACHO_CHECK_LT(shortWgs + longWgs, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT(numTasks + smallWgs, (int64_t)INT32_MAX);
  h.forChunks(batch, chunk, [&](int64_t q0, unsigned nm) {
    const hipk::FactorProductArgs<T> a{ls.at(q0), xs.at(q0), ys.at(q0), ldx, ldy, (int32_t)nRHS};
    if (!transposed) {
      hipk::factorProductLx<T><<<dim3((unsigned)(shortWgs + longWgs), nm, zGroups), hipk::kFpThreads, 0, stream>>>(
          pl, sk, (int32_t)order, (int32_t)shortWgs, (int32_t)numLong, a);
      if (numHuge > 0) {
        hipk::factorProductLxSpans<T><<<dim3((unsigned)numHuge, nm, zGroups), hipk::kFpSpanThreads, 0, stream>>>(pl, sk,
                                                                                                                a);
      }
      return;
    }
    T* part = reinterpret_cast<T*>(st.part.ptr);
    hipk::factorProductLt<T><<<dim3((unsigned)(numTasks + smallWgs), nm, zGroups), hipk::kFpThreads, 0, stream>>>(
        pl, sk, (int32_t)numTasks, (int32_t)numSmall, a, part, st.host.partElems);
    if (numFolds > 0) {
      hipk::factorProductLtFold<T><<<dim3((unsigned)((numFolds * 64 + hipk::kFpThreads - 1) / hipk::kFpThreads), nm,
                                          (unsigned)nRHS),
                                     hipk::kFpThreads, 0, stream>>>(pl.ltFolds, (int32_t)numFolds, a.y, ldy,
                                                                    (int32_t)nRHS, part, st.host.partElems);
    }
  });
}

#define BSP_INSTANTIATE_EXTENSIONS(T)                                                                            \
  template void hipBackendSelectedInverse<T>(SymbolicCtx&, T* const*, int64_t, bool);                           \
  template void hipBackendLogDet<T>(SymbolicCtx&, const T* const*, int64_t, bool, T*);                          \
  template void hipBackendPatternGrad<T>(SymbolicCtx&, const HipGradArgs<T>&, int64_t, bool);                   \
  template void hipBackendFactorStatus<T>(SymbolicCtx&, const T* const*, int64_t, bool, int64_t, int64_t,       \
                                          int64_t*);                                                            \
  template void hipBackendDampDiagonal<T>(SymbolicCtx&, T* const*, int64_t, bool, int64_t, int64_t, const T*);  \
  template void hipBackendFactorAdjointUpTo<T>(SymbolicCtx&, const T* const*, T* const*, int64_t, bool, int64_t); \
  template void hipBackendSelectedInverseAdjoint<T>(SymbolicCtx&, const T* const*, const T* const*, T* const*,  \
                                                    int64_t, bool);                                             \
  template void hipBackendSchurDense<T>(SymbolicCtx&, const T* const*, T* const*, int64_t, bool, int64_t,       \
                                        const int32_t*, bool);                                                  \
  template void hipBackendAssemble<T>(SymbolicCtx&, const AssemblyMap&, const T* const*, T* const*, int64_t,    \
                                      bool, bool);                                                              \
  template void hipBackendNormalEq<T>(SymbolicCtx&, const NormalEqMap&, int32_t, const T* const*,               \
                                      const T* const*, T* const*, int64_t, int64_t, bool);                      \
  template void hipBackendSymProduct<T>(SymbolicCtx&, const SymProductMap&, int32_t, const T* const*,           \
                                        const T* const*, T* const*, int64_t, int64_t, bool);                    \
  template void hipBackendSymResidual<T>(SymbolicCtx&, const SymProductMap&, const T* const*, const T* const*,  \
                                         const T* const*, T* const*, T* const*, int64_t, int64_t, bool);        \
  template void hipBackendColMax<T>(SymbolicCtx&, const T* const*, const T* const*, int64_t, int64_t, double*,  \
                                    int64_t, bool);                                                             \
  template void hipBackendNormEstStep<T>(SymbolicCtx&, int32_t, void*, const T* const*, int64_t*, double*,      \
                                         int64_t, bool);                                                        \
  template void hipBackendCg<T>(SymbolicCtx&, const CgArgs<T>&, int64_t, bool);                                 \
  template void hipBackendCgls<T>(SymbolicCtx&, const CglsArgs<T>&, int64_t, bool);                             \
  template void hipBackendJacSchur<T>(SymbolicCtx&, const JacSchurArgs<T>&, int64_t, bool);                     \
  template void hipBackendLanczos<T>(SymbolicCtx&, const LanczosArgs<T>&, int64_t, bool);                       \
  template void hipBackendKrylovCombine<T>(SymbolicCtx&, const KrylovCombineArgs<T>&, int64_t, bool);           \
  template void hipBackendReachSolveL<T>(SymbolicCtx&, const ReachPlan&, const T*, T*);                         \
  template void hipBackendGramBlocks<T>(SymbolicCtx&, const ReachPlan&, const T*, T*);                          \
  template T* hipBackendReachWorkspace<T>(SymbolicCtx&, int64_t);                                               \
  template void hipBackendFactorProduct<T>(SymbolicCtx&, const T* const*, bool, const T* const*, int64_t,       \
                                           T* const*, int64_t, int, int64_t, bool);
BSP_INSTANTIATE_EXTENSIONS(double)
BSP_INSTANTIATE_EXTENSIONS(float)
#undef BSP_INSTANTIATE_EXTENSIONS

}  // namespace BaSpaCho
