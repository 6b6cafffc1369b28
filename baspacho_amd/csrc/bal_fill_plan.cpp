// Host side of the ordered BAL fill: see bal_fill_plan.h.
#include "bal_fill_plan.h"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <tuple>

#include "entry_map.h"
#include "solver.h"

namespace BaSpaCho {

BalFillPlan::~BalFillPlan() {
  if (dev != nullptr) balFillPlanFreeDevice(dev);
}

template <typename U>
static int64_t bytesOf(const std::vector<U>& v) {
  return (int64_t)(v.size() * sizeof(U));
}

int64_t BalFillPlan::hostBytes() const {
  return bytesOf(ptPtr) + bytesOf(ptObs) + bytesOf(pairPtr) + bytesOf(pairCam) + bytesOf(pairPt) +
         bytesOf(pairStride) + bytesOf(pairFlip) + bytesOf(pairOff) + bytesOf(camPtr) + bytesOf(camObs) +
         bytesOf(camChunkPtr) + bytesOf(chunkCam) + bytesOf(chunkBegin) + bytesOf(chunkEnd) + bytesOf(ptDiagOff) +
         bytesOf(camDiagOff) + bytesOf(ptStart) + bytesOf(camStart) + bytesOf(ptDiagStride) + bytesOf(camDiagStride);
}

// (pairCam and pairPt stay on the host: the kernels need the block alone)
int64_t BalFillPlan::deviceBytes() const {
  return hostBytes() - bytesOf(pairCam) - bytesOf(pairPt) + scratchLen() * (int64_t)sizeof(double);
}

std::unique_ptr<BalFillPlan> createBalFillPlan(const Solver& solver, int camSize, int64_t numPts, int64_t numCams,
                                               int64_t numObs, const int64_t* obsCam, const int64_t* obsPt) {
  const std::string what = "bal fill plan: ";
  if (camSize != 9 && camSize != 6) throw std::runtime_error(what + "camera size must be 9 or 6");
  if (numPts < 0 || numCams < 0) throw std::runtime_error(what + "negative number of points or cameras");
  if (numObs < 0 || numObs >= ((int64_t)1 << 31)) {
    throw std::runtime_error(what + std::to_string(numObs) + " observations, must be in [0, 2^31)");
  }
  if (numPts + numCams != solver.skel().numSpans()) {
    throw std::runtime_error(what + std::to_string(numPts) + " points and " + std::to_string(numCams) +
                             " cameras for a solver of " + std::to_string(solver.skel().numSpans()) + " parameters");
  }
  const PermutedCoalescedAccessor acc = solver.accessor();
  for (int64_t p = 0; p < numPts + numCams; p++) {
    const int64_t want = p < numPts ? 3 : camSize;
    if (acc.paramSize(p) != want) {
      throw std::runtime_error(what + "parameter " + std::to_string(p) + " has size " +
                               std::to_string(acc.paramSize(p)) + ", the BAL layout needs " + std::to_string(want) +
                               " (points of size 3 first, then cameras of size " + std::to_string(camSize) + ")");
    }
  }
  if (solver.order() != 3 * numPts + camSize * numCams) {
    throw std::runtime_error(what + "the solver's order is " + std::to_string(solver.order()) + ", not 3 * " +
                             std::to_string(numPts) + " + " + std::to_string(camSize) + " * " +
                             std::to_string(numCams));
  }
  if (numObs > 0 && (obsCam == nullptr || obsPt == nullptr)) {
    throw std::runtime_error(what + "an observation list is NULL");
  }

  std::unique_ptr<BalFillPlan> plan(new BalFillPlan);
  BalFillPlan& m = *plan;
  m.solver = &solver;
  m.camSize = camSize;
  m.numPts = numPts;
  m.numCams = numCams;
  m.numObs = numObs;

  // kept observations in index order, then (camera, index) and (point, camera, index) by stable
  // counting sorts
  std::vector<int32_t> kept;
  for (int64_t o = 0; o < numObs; o++) {
    if (obsPt[o] >= 0 && obsPt[o] < numPts && obsCam[o] >= 0 && obsCam[o] < numCams) kept.push_back((int32_t)o);
  }
  m.numKept = (int64_t)kept.size();
  m.numSkipped = numObs - m.numKept;
  countingSort(kept, m.camObs, numCams, [obsCam](int32_t o) { return obsCam[o]; });
  countingSort(m.camObs, m.ptObs, numPts, [obsPt](int32_t o) { return obsPt[o]; });

  m.ptPtr.assign(numPts + 1, 0);
  m.camPtr.assign(numCams + 1, 0);
  for (int32_t o : kept) {
    m.ptPtr[obsPt[o] + 1]++;
    m.camPtr[obsCam[o] + 1]++;
  }
  for (int64_t p = 0; p < numPts; p++) {
    m.maxPtList = std::max<int64_t>(m.maxPtList, m.ptPtr[p + 1]);
    m.ptPtr[p + 1] += m.ptPtr[p];
  }
  for (int64_t c = 0; c < numCams; c++) {
    m.maxCamList = std::max<int64_t>(m.maxCamList, m.camPtr[c + 1]);
    m.camPtr[c + 1] += m.camPtr[c];
  }

  // pairs: runs of equal (point, camera) in ptObs, with the host accessor's answer for their block
  for (int64_t x = 0; x < m.numKept; x++) {
    const int32_t o = m.ptObs[x];
    const int64_t cam = obsCam[o], pt = obsPt[o];
    if (x > 0 && obsCam[m.ptObs[x - 1]] == cam && obsPt[m.ptObs[x - 1]] == pt) continue;
    const int64_t sc = solver.paramToSpan()[numPts + cam], sp = solver.paramToSpan()[pt];
    if (!acc.plainAcc.hasBlock(std::max(sc, sp), std::min(sc, sp))) {
      throw std::runtime_error(what + "observation " + std::to_string(o) + ": the block of camera " +
                               std::to_string(cam) + " and point " + std::to_string(pt) +
                               " is not in the solver's structure");
    }
    const auto osf = acc.blockOffset(numPts + cam, pt);
    m.pairPtr.push_back((int32_t)x);
    m.pairCam.push_back((int32_t)cam);
    m.pairPt.push_back((int32_t)pt);
    m.pairOff.push_back(std::get<0>(osf));
    m.pairStride.push_back((int32_t)std::get<1>(osf));
    m.pairFlip.push_back(std::get<2>(osf) ? 1 : 0);
  }
  m.pairPtr.push_back((int32_t)m.numKept);

  // chunks of every camera list
  m.camChunkPtr.assign(numCams + 1, 0);
  for (int64_t c = 0; c < numCams; c++) {
    for (int32_t b = m.camPtr[c]; b < m.camPtr[c + 1]; b += kBalFillChunk) {
      m.chunkCam.push_back((int32_t)c);
      m.chunkBegin.push_back(b);
      m.chunkEnd.push_back(std::min<int32_t>(b + kBalFillChunk, m.camPtr[c + 1]));
    }
    m.camChunkPtr[c + 1] = (int32_t)m.chunkCam.size();
  }

  // diagonal blocks and vector slices
  m.ptDiagOff.resize(numPts);
  m.ptDiagStride.resize(numPts);
  m.ptStart.resize(numPts);
  for (int64_t p = 0; p < numPts; p++) {
    const auto d = acc.diagBlockOffset(p);
    m.ptDiagOff[p] = d.first;
    m.ptDiagStride[p] = (int32_t)d.second;
    m.ptStart[p] = acc.paramStart(p);
  }
  m.camDiagOff.resize(numCams);
  m.camDiagStride.resize(numCams);
  m.camStart.resize(numCams);
  for (int64_t c = 0; c < numCams; c++) {
    const auto d = acc.diagBlockOffset(numPts + c);
    m.camDiagOff[c] = d.first;
    m.camDiagStride[c] = (int32_t)d.second;
    m.camStart[c] = acc.paramStart(numPts + c);
  }
  return plan;
}

}  // namespace BaSpaCho
