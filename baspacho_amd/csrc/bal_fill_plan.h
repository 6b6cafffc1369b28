// Plan of the ordered Hessian fill of the BAL pipeline (balFillOrdered, bal_pipeline.h; DESIGN.md
// section 9, "Ordered fill").  Built once per problem on the host from the observation list and the
// solver's accessor: the observations grouped by point and by camera, every (point, camera) pair with
// the block the accessor answers for it, and the camera lists cut into chunks.  The kernels read these
// tables only, so every sum they take runs in an order the plan fixes.  Host only, no device work; the
// device copy is made by the first balFillOrdered that uses the plan.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

namespace BaSpaCho {

class Solver;
struct BalFillPlanDev;  // the tables and the chunk scratch on the device (bal_pipeline.hip)

// constants of the build (bsp_bal_fill_plan_info reports them): a camera list is cut into chunks of
// kBalFillChunk consecutive list positions, and kBalFillLanes lanes share the sum of one element over
// a chunk
constexpr int kBalFillChunk = 128, kBalFillLanes = 4;

struct BalFillPlan {
  const Solver* solver = nullptr;  // the solver whose layout the plan targets
  int camSize = 0;
  int64_t numPts = 0, numCams = 0, numObs = 0;
  int64_t numKept = 0, numSkipped = 0;  // observations with both indices in range / left out
  int64_t maxPtList = 0, maxCamList = 0;

  // by point: the kept observations sorted by (point, camera, observation index); point p owns
  // ptObs[ptPtr[p] .. ptPtr[p + 1])
  std::vector<int32_t> ptPtr, ptObs;
  // pairs: pair q is the run ptObs[pairPtr[q] .. pairPtr[q + 1]) of equal (point, camera); its block
  // (numPts + pairCam[q], pairPt[q]) starts at pairOff[q] with row stride pairStride[q], stored
  // transposed when pairFlip[q]
  std::vector<int32_t> pairPtr, pairCam, pairPt, pairStride, pairFlip;
  std::vector<int64_t> pairOff;
  // by camera: the kept observations sorted by (camera, observation index); camera c owns
  // camObs[camPtr[c] .. camPtr[c + 1]) and the chunks camChunkPtr[c] .. camChunkPtr[c + 1]; chunk k
  // covers the list positions chunkBegin[k] .. chunkEnd[k] (positions into camObs) of chunkCam[k]
  std::vector<int32_t> camPtr, camObs, camChunkPtr, chunkCam, chunkBegin, chunkEnd;
  // diagonal blocks and vector slices, per point and per camera
  std::vector<int64_t> ptDiagOff, camDiagOff, ptStart, camStart;
  std::vector<int32_t> ptDiagStride, camDiagStride;

  mutable BalFillPlanDev* dev = nullptr;

  BalFillPlan() = default;
  BalFillPlan(const BalFillPlan&) = delete;
  BalFillPlan& operator=(const BalFillPlan&) = delete;
  ~BalFillPlan();

  int64_t numPairs() const { return (int64_t)pairOff.size(); }
  int64_t numChunks() const { return (int64_t)chunkCam.size(); }
  // words of one chunk partial: the lower triangle of the camera's diagonal block, then its gradient
  int64_t partialWords() const { return (int64_t)camSize * (camSize + 1) / 2 + camSize; }
  int64_t scratchLen() const { return numChunks() * partialWords(); }  // doubles
  int64_t hostBytes() const;
  int64_t deviceBytes() const;  // tables + scratch, once uploaded
};

// Builds the plan.  obsCam / obsPt are HOST arrays of numObs entries; an observation whose camera is
// outside [0, numCams) or whose point is outside [0, numPts) is left out and counted.  Throws, before
// it reads the lists, for a camera size other than 9 or 6, numObs outside [0, 2^31), and a solver that
// does not have numPts parameters of size 3 followed by numCams of size camSize (order 3 numPts +
// camSize numCams); and for a kept observation whose block (numPts + cam, pt) the solver does not store.
// Counting sorts only.
std::unique_ptr<BalFillPlan> createBalFillPlan(const Solver& solver, int camSize, int64_t numPts, int64_t numCams,
                                               int64_t numObs, const int64_t* obsCam, const int64_t* obsPt);

// the device copy of a plan is released by bal_pipeline.hip
void balFillPlanFreeDevice(BalFillPlanDev* dev);

}  // namespace BaSpaCho
