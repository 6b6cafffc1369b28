// Device-side caller pipeline of the BAL benchmark (see bal_pipeline.hip): residuals + Jacobians of
// every observation, and Hessian / gradient assembly through the device accessor.
#pragma once

#include <cstdint>

#include "accessor.h"
#include "bal_fill_plan.h"

namespace BaSpaCho {

// res[2 nObs], Jc[nObs][2][9], Jp[nObs][2][3] (all device, fp64); cams[nCams][9], pts[nPts][3]
void balLinearize(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                  const double* cams, const double* pts, double* res, double* Jc, double* Jp,
                  void* stream);

// the same in the reference's parameterisation (BaAtLarge.h:56-150): camera = SE(3) tangent of a left
// perturbation (translation, rotation), calibration fixed; Jc[nObs][2][6]
void balLinearizeSe3(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                     const double* cams, const double* pts, double* res, double* Jc, double* Jp,
                     void* stream);

// data += J^T J block by block (data must have been zeroed by the caller), grad += J^T r (optional),
// then every diagonal entry d <- d (1 + lambda) + 1e-3 lambda.  acc = Solver::deviceAccessor();
// caller's parameter numbering: points first, cameras after.  dbg (optional, 7 int64 per
// observation): the offsets / strides / flip the accessor returned.
// camSize: 9 (BAL file parameters, Jc[.][2][9]) or 6 (SE3 tangent, Jc[.][2][6])
template <typename T>
void balFillHessian(const PermutedCoalescedAccessor& acc, int camSize, int64_t numPts, int64_t numCams,
                    int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* Jc,
                    const double* Jp, const double* res, T lambda, T* data, T* grad, int64_t* dbg,
                    void* stream);

// ---- ordered fill: the contract of balFillHessian (data += J^T J on the blocks the observations map
// to, diagonal blocks in full, off-diagonal blocks once and transposed where the accessor says so; grad
// += J^T r, grad may be NULL; then d <- d (1 + lambda) + 1e-3 lambda on every diagonal entry unless
// lambda == 0) without atomics: every sum is taken in an order that the plan alone fixes
// (bal_fill_plan.h), so data and grad are the same bits on every run and every device.  Launches go to
// `stream`; nothing synchronises the host.  The first call with a plan uploads its tables (one
// allocation, one blocking copy); later calls allocate nothing.  The chunk partials live in the plan's
// own scratch, so one plan serves one call at a time (calls on one stream are ordered).
//
// SUMMATION ORDER.  J0, J1 are the two residual rows of an observation, r0, r1 its residuals; fl() is
// one fp64 rounding and nothing is fused.
//   term of observation o for columns a, b:   fl(fl(J0a * J0b) + fl(J1a * J1b))
//   gradient term of column a:                fl(fl(J0a * r0) + fl(J1a * r1))
//   pair block (camera c, point p), element (i, j): S = +0.0, then S = fl(S + term(Jc_i, Jp_j)) over the
//     pair's run of ptObs, in list order
//   point block element (i, j) and point gradient entry i: the same left fold over the point's list
//     ptObs[ptPtr[p] .. ptPtr[p + 1])
//   camera block element (a, b), a >= b, and camera gradient entry a: for every chunk of the camera's
//     list, lane l < W = kBalFillLanes folds the terms at the chunk positions l, l + W, l + 2 W, .. from
//     +0.0; then for h = W / 2, .., 1: T[l] = fl(T[l] + T[l + h]) for l < h; the chunk's partial is T[0].
//     S = +0.0, then S = fl(S + partial) over the camera's chunks in chunk order.  Element (b, a) gets
//     the sum of (a, b) (fl(x * y) == fl(y * x), so it is its own sum too).
//   applied once per element: data[e] = data[e] + (T)S in T arithmetic (likewise grad); an element no
//     kept observation maps to is not written.
template <typename T>
void balFillOrdered(const BalFillPlan& plan, const double* Jc, const double* Jp, const double* res, T lambda,
                    T* data, T* grad, void* stream);

// ---- the rest of a Levenberg-Marquardt iteration ("LM step on the device").
// All pointers are device memory, everything is fp64; nothing here uses atomics, synchronises the host
// or allocates, and every launch goes to `stream`.

// the residuals alone, res[2 nObs], in plain doubles: what balLinearize / balLinearizeSe3 write to res
// (the SE3 form with the same behind-the-camera rule: camPt.z > 0.01 gives exactly (25, 0))
void balResiduals(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                  const double* cams, const double* pts, double* res, void* stream);
void balResidualsSe3(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                     const double* cams, const double* pts, double* res, void* stream);

// Robust loss (examples/SoftLoss.h jet2, examples/Optimizer.h computeSingleGradHess): per observation
// s = r0^2 + r1^2, rho[o] = rho(s), w = rho'(s).
//   kind 0 trivial: (s, 1);  1 Huber: s > a^2 ? (2 a sqrt(s) - a^2, a / sqrt(s)) : (s, 1);
//   2 Cauchy: (a^2 log1p(s / a^2), 1 / (1 + s / a^2))
// With Jc and Jp given (both or neither), the observation's 2 residuals and its 2 x camSize and 2 x 3
// Jacobian rows are multiplied in place by sqrt(w), so that balFillHessian accumulates w J^T J and
// w J^T r (no second-order term, as in the reference); the words of an observation with w == 1 are not
// written.  With Jc = Jp = NULL only rho is written (res is read only).  Throws, before any launch, for
// an unknown kind or an `a` that is not finite and positive.
void balLoss(int64_t numObs, int camSize, int kind, double a, double* res, double* Jc, double* Jp,
             double* rho, void* stream);

// out[0] = scale * sum_{i < n} x[i] in a fixed order (bitwise reproducible), +0.0 for n == 0.
// scratch: balSumScratchLen(n) = ceil(n / 2048) doubles.  Order: chunk b = x[2048 b, 2048 (b + 1));
// thread sums T[t] = ((0 + x[2048 b + t]) + x[2048 b + 256 + t]) + .. (8 terms, those below n); fold
// for s = 128, 64, .. 1: T[t] += T[t + s] for t < s; part[b] = T[0].  Then the same with
// T[t] = ((0 + part[t]) + part[t + 256]) + .. and out[0] = scale * T[0].
int64_t balSumScratchLen(int64_t n);
void balSum(int64_t n, const double* x, double scale, double* scratch, double* out, void* stream);

// applyStep of the reference's optimizer (BaAtLargeOptimizer.cpp:173-184), out of place: camsOut /
// ptsOut must not overlap cams / pts / step.  `step` is in the solver's internal order (what solve()
// leaves in the gradient buffer); parameter p's slice starts at acc.paramStart(p), points first, cameras
// after.  ptsOut = pts - step.  balApplyStep: all 9 camera parameters minus their slice.
// balApplyStepSe3: T <- exp(-step) T with step = (u, w), translation first; rotations composed as unit
// quaternions and returned as an axis-angle vector with |w| <= pi; (f, k1, k2) copied.
void balApplyStep(const PermutedCoalescedAccessor& acc, int64_t numPts, int64_t numCams, const double* cams,
                  const double* pts, const double* step, double* camsOut, double* ptsOut, void* stream);
void balApplyStepSe3(const PermutedCoalescedAccessor& acc, int64_t numPts, int64_t numCams,
                     const double* cams, const double* pts, const double* step, double* camsOut,
                     double* ptsOut, void* stream);

}  // namespace BaSpaCho
