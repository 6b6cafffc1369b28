// Caller pipeline of the bundle-adjustment-at-large benchmark on the device: linearisation of the
// reprojection residuals and assembly of the Gauss-Newton Hessian / gradient straight into the
// solver's numeric buffer through Solver::deviceAccessor() -- what the reference's optimizer does on
// the host in its computeStep (benchmarking/BaAtLargeOptimizer.cpp:100-131: accessor.diagBlock /
// accessor.block per observation, then the Levenberg-Marquardt damping of every diagonal) and what
// its CUDA backend offers the accessor for (Accessor.h:110-200 is host/device, MatOpsCuda.cu:85-92
// hands out the device arrays).  Cameras carry the 9 parameters of a BAL file (Rodrigues rotation,
// translation, f, k1, k2 -- the block size BAL_bench uses, BaAtLargeBench.cpp:50-65); the
// derivatives come from forward-mode dual numbers, so there is no hand-derived Jacobian to get wrong.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "accessor.h"
#include "bal_fill_kernels.h"
#include "bal_pipeline.h"
#include "solver.h"

namespace BaSpaCho {

namespace {

#define balCHECK(expr)                                                                      \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #expr); \
    }                                                                                       \
  } while (0)

constexpr int kND = 12;  // 9 camera + 3 point partials

struct Dual {
  double v;
  double d[kND];
};
__device__ __forceinline__ Dual constant(double v) {
  Dual r;
  r.v = v;
#pragma unroll
  for (int i = 0; i < kND; i++) r.d[i] = 0.0;
  return r;
}
__device__ __forceinline__ Dual variable(double v, int idx) {
  Dual r = constant(v);
  r.d[idx] = 1.0;
  return r;
}
__device__ __forceinline__ Dual operator+(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < kND; i++) r.d[i] = a.d[i] + b.d[i];
  return r;
}
__device__ __forceinline__ Dual operator-(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < kND; i++) r.d[i] = a.d[i] - b.d[i];
  return r;
}
__device__ __forceinline__ Dual operator*(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < kND; i++) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
__device__ __forceinline__ Dual operator/(const Dual& a, const Dual& b) {
  Dual r;
  const double inv = 1.0 / b.v;
  r.v = a.v * inv;
#pragma unroll
  for (int i = 0; i < kND; i++) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
__device__ __forceinline__ Dual scale(const Dual& a, double s, double ds_dv) {
  // f(a) with f(a.v) = s and f'(a.v) = ds_dv
  Dual r;
  r.v = s;
#pragma unroll
  for (int i = 0; i < kND; i++) r.d[i] = ds_dv * a.d[i];
  return r;
}

// a(x) = sin(sqrt x) / sqrt x = sum (-x)^k / (2k+1)!,  b(x) = (1 - cos(sqrt x)) / x = sum (-x)^k / (2k+2)!
// and their derivatives in x = theta^2.  The closed forms of the derivatives,
//   a' = (theta cos(theta) - sin(theta)) / (2 theta^3),  b' = (theta sin(theta) - 2 (1 - cos(theta))) / (2 theta^4),
// cancel: their relative errors are about 3 eps / x and 12 eps / x.  Below the cut a and b are their
// degree-6 polynomials (truncation x^7 / 15! relative) and a', b' the exact derivatives of those, six
// terms each, truncated at 42 x^6 / 15! and 168 x^6 / 16! relative.  The two error curves cross at
// x = 0.19 (a') and x = 0.29 (b'); the cut is x = 0.25 (theta = 0.5), where the closed forms are off by
// 1.3e-15 and 5.3e-15 and the series by 7.8e-15 and 1.9e-15 -- on terms that enter the Jacobian scaled by
// x / 3 or less.  Above the cut b = 2 sin^2(theta / 2) / theta^2, which does not cancel at all.
constexpr double kRotationSeriesCut = 0.25;
__device__ __forceinline__ void rotationCoefficients(double x, double& a, double& b, double& da,
                                                     double& db) {
  if (x >= kRotationSeriesCut) {
    const double th = sqrt(x), s = sin(th), c = cos(th), sh = sin(0.5 * th);
    a = s / th;
    b = 2.0 * sh * sh / x;
    da = (th * c - s) / (2.0 * th * x);
    db = (th * s - 4.0 * sh * sh) / (2.0 * x * x);
  } else {
    // 1 / (2k+1)! and 1 / (2k+2)!, k = 0..6
    constexpr double ca[7] = {1.0, 1.0 / 6, 1.0 / 120, 1.0 / 5040, 1.0 / 362880, 1.0 / 39916800,
                              1.0 / 6227020800.0};
    constexpr double cb[7] = {1.0 / 2, 1.0 / 24, 1.0 / 720, 1.0 / 40320, 1.0 / 3628800, 1.0 / 479001600,
                              1.0 / 87178291200.0};
    const double y = -x;
    a = ca[6];
    b = cb[6];
    da = 6.0 * ca[6];
    db = 6.0 * cb[6];
#pragma unroll
    for (int k = 5; k >= 0; k--) {
      a = a * y + ca[k];
      b = b * y + cb[k];
      if (k >= 1) {
        da = da * y + k * ca[k];
        db = db * y + k * cb[k];
      }
    }
    da = -da;  // d/dx of sum c_k (-x)^k = -sum k c_k (-x)^(k-1)
    db = -db;
  }
}

// residual (2) and its derivatives for one observation; camera = [r(3), t(3), f, k1, k2]
__device__ __forceinline__ void reproject(const double* cam, const double* pt, const double* xy,
                                          Dual (&res)[2]) {
  Dual w[3], t[3], X[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    w[i] = variable(cam[i], i);
    t[i] = variable(cam[3 + i], 3 + i);
    X[i] = variable(pt[i], 9 + i);
  }
  const Dual f = variable(cam[6], 6), k1 = variable(cam[7], 7), k2 = variable(cam[8], 8);
  // Rodrigues rotation of X by the axis-angle vector w, through smooth functions of x = theta^2:
  //   R X = X + a (w x X) + b (w x (w x X)),  a = sin(theta) / theta,  b = (1 - cos(theta)) / theta^2.
  // No 1 / theta enters the dual path (the axis w / theta has derivatives of size 1 / theta, whose
  // rounding errors made the rotation columns lose accuracy like eps / theta).
  const Dual th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double a, b, da, db;  // a(x), b(x) and their derivatives in x
  rotationCoefficients(th2.v, a, b, da, db);
  const Dual A = scale(th2, a, da), B = scale(th2, b, db);
  const Dual wX[3] = {w[1] * X[2] - w[2] * X[1], w[2] * X[0] - w[0] * X[2], w[0] * X[1] - w[1] * X[0]};
  const Dual wwX[3] = {w[1] * wX[2] - w[2] * wX[1], w[2] * wX[0] - w[0] * wX[2],
                       w[0] * wX[1] - w[1] * wX[0]};
  Dual P[3];
#pragma unroll
  for (int i = 0; i < 3; i++) P[i] = X[i] + A * wX[i] + B * wwX[i];
#pragma unroll
  for (int i = 0; i < 3; i++) P[i] = P[i] + t[i];
  const Dual zero = constant(0.0);
  const Dual px = (zero - P[0]) / P[2], py = (zero - P[1]) / P[2];
  const Dual r2 = px * px + py * py;
  const Dual dist = constant(1.0) + r2 * (k1 + k2 * r2);
  res[0] = f * dist * px - constant(xy[0]);
  res[1] = f * dist * py - constant(xy[1]);
}

__global__ __launch_bounds__(64) void balLinearizeKernel(int64_t numObs, const int64_t* obsCam,
                                                         const int64_t* obsPt, const double* obsXy,
                                                         const double* cams, const double* pts,
                                                         double* res, double* Jc, double* Jp) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= numObs) return;
  Dual r[2];
  reproject(cams + 9 * obsCam[o], pts + 3 * obsPt[o], obsXy + 2 * o, r);
#pragma unroll
  for (int e = 0; e < 2; e++) {
    res[2 * o + e] = r[e].v;
#pragma unroll
    for (int i = 0; i < 9; i++) Jc[18 * o + 9 * e + i] = r[e].d[i];
#pragma unroll
    for (int i = 0; i < 3; i++) Jp[6 * o + 3 * e + i] = r[e].d[9 + i];
  }
}

// The REFERENCE's parameterisation (benchmarking/BaAtLarge.h:56-150, Cost::compute_residual as the
// LM optimizer calls it, BaAtLargeOptimizer.cpp:108-124): the camera is T_W_C in SE(3) (camPt = R X +
// t) with FIXED calibration (f, k1, k2); its 6 parameters are the tangent of a LEFT perturbation,
// translation first, T <- exp(delta) T, and the optimizer applies T <- exp(-step) T
// (BaAtLargeOptimizer.cpp:176-183).  Jacobians in closed form, exactly the expressions of the
// reference: with p = -camPt.xy / camPt.z, s = |p|^2, r = 1 + (k1 + k2 s) s,
//   D = d p / d(.) ,   J = f r D + p (2 p^T D) f (k1 + 2 k2 s),
// D_point = [(z R_0 - x R_2); (z R_1 - y R_2)] * (-1 / z^2),  D_cam = the 2 x 6 matrix below.
// A point in front of the image plane (camPt.z > 0.01; BAL cameras look down -z) gives the fixed
// residual (25, 0) and zero Jacobians, as in the reference.
__device__ __forceinline__ void rodriguesMatrix(const double* w, double (&R)[3][3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double a, b;  // R = I + a [w]x + b [w]x^2
  if (th2 > 1e-20) {
    const double th = sqrt(th2);
    a = sin(th) / th;
    b = (1.0 - cos(th)) / th2;
  } else {
    a = 1.0;
    b = 0.5;
  }
  const double K[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double k2 = 0;
#pragma unroll
      for (int l = 0; l < 3; l++) k2 += K[i][l] * K[l][j];
      R[i][j] = (i == j ? 1.0 : 0.0) + a * K[i][j] + b * k2;
    }
  }
}

__global__ __launch_bounds__(64) void balLinearizeSe3Kernel(int64_t numObs, const int64_t* obsCam,
                                                            const int64_t* obsPt, const double* obsXy,
                                                            const double* cams, const double* pts,
                                                            double* res, double* Jc, double* Jp) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= numObs) return;
  const double* cam = cams + 9 * obsCam[o];
  const double* X = pts + 3 * obsPt[o];
  double R[3][3];
  rodriguesMatrix(cam, R);
  double P[3];
#pragma unroll
  for (int i = 0; i < 3; i++) P[i] = R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + cam[3 + i];
  double* jc = Jc + 12 * o;
  double* jp = Jp + 6 * o;
  if (P[2] > 0.01) {
    res[2 * o] = 25.0;
    res[2 * o + 1] = 0.0;
#pragma unroll
    for (int i = 0; i < 12; i++) jc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) jp[i] = 0.0;
    return;
  }
  const double f = cam[6], k1 = cam[7], k2 = cam[8];
  const double p0 = -P[0] / P[2], p1 = -P[1] / P[2];
  const double sq = p0 * p0 + p1 * p1;
  const double r = 1.0 + (k1 + k2 * sq) * sq;
  res[2 * o] = f * r * p0 - obsXy[2 * o];
  res[2 * o + 1] = f * r * p1 - obsXy[2 * o + 1];
  const double g = f * (k1 + k2 * 2.0 * sq);
  // point Jacobian
  {
    const double denum = -1.0 / (P[2] * P[2]);
    double D[2][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      D[0][c] = (P[2] * R[0][c] - P[0] * R[2][c]) * denum;
      D[1][c] = (P[2] * R[1][c] - P[1] * R[2][c]) * denum;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double dsq = 2.0 * (p0 * D[0][c] + p1 * D[1][c]);
      jp[c] = f * r * D[0][c] + p0 * dsq * g;
      jp[3 + c] = f * r * D[1][c] + p1 * dsq * g;
    }
  }
  // camera Jacobian (translation, rotation)
  {
    const double dz = 1.0 / P[2], xdz = P[0] * dz, ydz = P[1] * dz, xydz2 = xdz * ydz;
    const double D[2][6] = {{-dz, 0.0, xdz * dz, xydz2, -1.0 - xdz * xdz, ydz},
                            {0.0, -dz, ydz * dz, 1.0 + ydz * ydz, -xydz2, -xdz}};
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const double dsq = 2.0 * (p0 * D[0][c] + p1 * D[1][c]);
      jc[c] = f * r * D[0][c] + p0 * dsq * g;
      jc[6 + c] = f * r * D[1][c] + p1 * dsq * g;
    }
  }
}

// One observation per 64 threads (a wave): H(cam,cam) += Jc^T Jc, H(pt,pt) += Jp^T Jp,
// H(cam,pt) += Jc^T Jp, g += J^T r -- every block located with the device accessor.
// Parameter numbering of the caller: points 0..numPts-1, cameras numPts.. (BaAtLargeBench.cpp:50-57).
template <typename T>
__global__ __launch_bounds__(256) void balFillKernel(PermutedCoalescedAccessor acc, int camSize,
                                                     int64_t numPts, int64_t numCams,
                                                     int64_t numObs, const int64_t* obsCam,
                                                     const int64_t* obsPt, const double* Jc,
                                                     const double* Jp, const double* res, T* data,
                                                     T* grad, int64_t* dbg) {
  const int lane = threadIdx.x & 63;
  const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= numObs) return;
  // (an observation whose indices fall outside [0, numPts) x [0, numCams) is skipped: its atomics
  //  would land outside the numeric data; the host-side loader rejects such files, bal.py)
  if (obsPt[o] < 0 || obsPt[o] >= numPts || obsCam[o] < 0 || obsCam[o] >= numCams) return;
  const int64_t ptId = obsPt[o], camId = numPts + obsCam[o];
  const int CS = camSize;  // camera block: 9 (BAL file parameters) or 6 (SE3 tangent)
  const double* jc = Jc + 2 * CS * o;
  const double* jp = Jp + 6 * o;
  // off-diagonal block (cam, pt): 9 x 3, stored as it is or transposed (flipped)
  const auto off = acc.blockOffset(camId, ptId);
  const int64_t bo = std::get<0>(off), bs = std::get<1>(off);
  const bool flip = std::get<2>(off);
  if (lane < 3 * CS) {
    const int i = lane / 3, j = lane % 3;  // (camera row, point column)
    const double v = jc[i] * jp[j] + jc[CS + i] * jp[3 + j];
    T* p = data + bo + (flip ? (int64_t)j * bs + i : (int64_t)i * bs + j);
    unsafeAtomicAdd(p, (T)v);
  }
  // diagonal blocks (lower AND upper triangle written, as Eigen's += on the full block does)
  const auto dc = acc.diagBlockOffset(camId);
  for (int e = lane; e < CS * CS; e += 64) {
    const int i = e / CS, j = e % CS;
    unsafeAtomicAdd(data + dc.first + (int64_t)i * dc.second + j,
                    (T)(jc[i] * jc[j] + jc[CS + i] * jc[CS + j]));
  }
  const auto dp = acc.diagBlockOffset(ptId);
  if (lane < 9) {
    const int i = lane / 3, j = lane % 3;
    unsafeAtomicAdd(data + dp.first + (int64_t)i * dp.second + j,
                    (T)(jp[i] * jp[j] + jp[3 + i] * jp[3 + j]));
  }
  if (grad) {
    const double r0 = res[2 * o], r1 = res[2 * o + 1];
    if (lane < CS) unsafeAtomicAdd(grad + acc.paramStart(camId) + lane, (T)(jc[lane] * r0 + jc[CS + lane] * r1));
    if (lane >= 16 && lane < 19) {
      const int i = lane - 16;
      unsafeAtomicAdd(grad + acc.paramStart(ptId) + i, (T)(jp[i] * r0 + jp[3 + i] * r1));
    }
  }
  if (dbg && lane == 0) {  // what the accessor answered, for the integer parity test
    int64_t* d = dbg + 7 * o;
    d[0] = bo;
    d[1] = bs;
    d[2] = flip ? 1 : 0;
    d[3] = dc.first;
    d[4] = dc.second;
    d[5] = dp.first;
    d[6] = dp.second;
  }
}

// Levenberg-Marquardt damping of every diagonal entry (BaAtLargeOptimizer.cpp:126-130)
template <typename T>
__global__ __launch_bounds__(256) void balDampKernel(PermutedCoalescedAccessor acc, int64_t numParams,
                                                     T lambda, T* data) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= numParams) return;
  const auto d = acc.diagBlockOffset(p);
  const int64_t n = acc.paramSize(p);
  for (int64_t i = 0; i < n; i++) {
    T* e = data + d.first + i * (d.second + 1);
    *e = *e * (T(1) + lambda) + lambda * T(1e-3);
  }
}

// ---- the rest of a Levenberg-Marquardt iteration: candidate cost, robust loss, retraction ----------
// (conventions, summation order, tolerances and resource usage: DESIGN.md section 9, "LM step on the
//  device").  None of these kernels uses atomics; every sum runs in a fixed order.

// Residual of the 9-parameter camera in plain doubles: reproject() without its 12 dual parts, through
// the same rotationCoefficients (no w / theta).
__global__ __launch_bounds__(256) void balResidualsKernel(int64_t numObs, const int64_t* obsCam,
                                                          const int64_t* obsPt, const double* obsXy,
                                                          const double* cams, const double* pts,
                                                          double* res) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= numObs) return;
  const double* cam = cams + 9 * obsCam[o];
  const double* X = pts + 3 * obsPt[o];
  const double w[3] = {cam[0], cam[1], cam[2]};
  double a, b, da, db;
  rotationCoefficients(w[0] * w[0] + w[1] * w[1] + w[2] * w[2], a, b, da, db);
  const double wX[3] = {w[1] * X[2] - w[2] * X[1], w[2] * X[0] - w[0] * X[2], w[0] * X[1] - w[1] * X[0]};
  const double wwX[3] = {w[1] * wX[2] - w[2] * wX[1], w[2] * wX[0] - w[0] * wX[2],
                         w[0] * wX[1] - w[1] * wX[0]};
  double P[3];
#pragma unroll
  for (int i = 0; i < 3; i++) P[i] = X[i] + a * wX[i] + b * wwX[i] + cam[3 + i];
  const double inv = 1.0 / P[2], px = -P[0] * inv, py = -P[1] * inv;
  const double r2 = px * px + py * py;
  const double fd = cam[6] * (1.0 + r2 * (cam[7] + cam[8] * r2));
  res[2 * o] = fd * px - obsXy[2 * o];
  res[2 * o + 1] = fd * py - obsXy[2 * o + 1];
}

// Residual of the SE3 parameterisation: the residual part of balLinearizeSe3Kernel, statement for
// statement (same rodriguesMatrix, same behind-the-camera rule), so that the cost of a candidate and the
// cost at a linearisation point are the same function of the parameters.
__global__ __launch_bounds__(256) void balResidualsSe3Kernel(int64_t numObs, const int64_t* obsCam,
                                                             const int64_t* obsPt, const double* obsXy,
                                                             const double* cams, const double* pts,
                                                             double* res) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= numObs) return;
  const double* cam = cams + 9 * obsCam[o];
  const double* X = pts + 3 * obsPt[o];
  double R[3][3];
  rodriguesMatrix(cam, R);
  double P[3];
#pragma unroll
  for (int i = 0; i < 3; i++) P[i] = R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + cam[3 + i];
  if (P[2] > 0.01) {
    res[2 * o] = 25.0;
    res[2 * o + 1] = 0.0;
    return;
  }
  const double f = cam[6], k1 = cam[7], k2 = cam[8];
  const double p0 = -P[0] / P[2], p1 = -P[1] / P[2];
  const double sq = p0 * p0 + p1 * p1;
  const double r = 1.0 + (k1 + k2 * sq) * sq;
  res[2 * o] = f * r * p0 - obsXy[2 * o];
  res[2 * o + 1] = f * r * p1 - obsXy[2 * o + 1];
}

// Robust loss (examples/SoftLoss.h: jet2 of TrivialLoss / HuberLoss / CauchyLoss, applied as in
// examples/Optimizer.h computeSingleGradHess).  A workgroup owns kBalLossTile consecutive observations.
// Pass 1, one thread per observation: s = |r|^2, rho[o] = rho(s), sqrt(rho'(s)) into LDS.  Pass 2: the
// tile's words of Jc, Jp and res are walked flat across the lanes (word e belongs to observation
// e / wordsPerObs of the tile), so consecutive lanes store consecutive words; a word whose weight is
// exactly 1 is not stored at all.  res is read in pass 1 and rewritten in pass 2 by the same workgroup
// only, with a barrier in between.
constexpr int kBalLossTile = 256;
template <int CS>  // camera block width, 9 or 6
__global__ __launch_bounds__(kBalLossTile) void balLossKernel(int64_t numObs, int kind, double a,
                                                              double* res, double* Jc, double* Jp,
                                                              double* rho) {
  __shared__ double sw[kBalLossTile];
  const int tid = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * kBalLossTile, o = o0 + tid;
  double sq = 1.0;
  if (o < numObs) {
    const double r0 = res[2 * o], r1 = res[2 * o + 1];
    const double s = r0 * r0 + r1 * r1, a2 = a * a;
    double v = s;
    if (kind == 1) {
      if (s > a2) {
        const double r = sqrt(s);
        v = 2.0 * a * r - a2;
        sq = sqrt(a / r);
      }
    } else if (kind == 2) {
      const double x = s / a2;
      v = a2 * log1p(x);
      sq = sqrt(1.0 / (1.0 + x));
    }
    rho[o] = v;
  }
  if (Jc == nullptr) return;
  sw[tid] = sq;
  __syncthreads();
  const int64_t left = numObs - o0;
  const int nObs = left < kBalLossTile ? (int)left : kBalLossTile;
  double* jc = Jc + 2 * CS * o0;
  for (int e = tid; e < 2 * CS * nObs; e += kBalLossTile) {
    const double f = sw[e / (2 * CS)];
    if (f != 1.0) jc[e] *= f;
  }
  double* jp = Jp + 6 * o0;
  for (int e = tid; e < 6 * nObs; e += kBalLossTile) {
    const double f = sw[e / 6];
    if (f != 1.0) jp[e] *= f;
  }
  double* rr = res + 2 * o0;
  for (int e = tid; e < 2 * nObs; e += kBalLossTile) {
    const double f = sw[e / 2];
    if (f != 1.0) rr[e] *= f;
  }
}

// Fixed-order sum, out[0] = scale * sum x, in two passes (the pattern of logDetPartial / logDetFinal).
// Pass 1: workgroup b of 256 threads owns x[b * kBalSumChunk, (b + 1) * kBalSumChunk).  Thread t adds, in
// this order and starting from +0.0, the elements b * kBalSumChunk + m * 256 + t, m = 0 .. 7, that exist.
// The 256 thread sums are then folded in LDS: for s = 128, 64, .. 1, entry t < s becomes entry t + entry
// t + s.  Entry 0 is part[b].
// Pass 2: one workgroup.  Thread t adds part[t], part[t + 256], .. in this order from +0.0; the same fold;
// out[0] = scale * entry 0 (+0.0 when there are no partial sums).
constexpr int kBalSumChunk = 2048, kBalSumWidth = 256;
__global__ __launch_bounds__(kBalSumWidth) void balSumPartial(int64_t n, const double* x, double* part) {
  __shared__ double red[kBalSumWidth];
  const int tid = threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int m = 0; m < kBalSumChunk / kBalSumWidth; m++) {
    const int64_t g = (int64_t)blockIdx.x * kBalSumChunk + m * kBalSumWidth + tid;
    if (g < n) acc += x[g];
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = kBalSumWidth / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kBalSumWidth) void balSumFinal(int64_t nParts, const double* part,
                                                           double scale, double* out) {
  __shared__ double red[kBalSumWidth];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t b = tid; b < nParts; b += kBalSumWidth) acc += part[b];
  red[tid] = acc;
  __syncthreads();
  for (int s = kBalSumWidth / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[0] = nParts > 0 ? scale * red[0] : 0.0;
}

// c(x) = (theta - sin(theta)) / theta^3 = sum (-x)^k / (2k+3)!, x = theta^2: the second coefficient of
// V = I + b [w]x + c [w]x^2 (Sophus::SE3d::exp).  The closed form cancels like 6 eps / x; below x = 1 the
// nine-term series (truncation 6 x^9 / 21! = 1.2e-19 relative at the cut) replaces it.
__device__ __forceinline__ double translationCoefficient(double x) {
  if (x >= 1.0) {
    const double th = sqrt(x);
    return (th - sin(th)) / (th * x);
  }
  constexpr double cc[9] = {1.0 / 6,
                            1.0 / 120,
                            1.0 / 5040,
                            1.0 / 362880,
                            1.0 / 39916800,
                            1.0 / 6227020800.0,
                            1.0 / 1307674368000.0,
                            1.0 / 355687428096000.0,
                            1.0 / 121645100408832000.0};
  const double y = -x;
  double c = cc[8];
#pragma unroll
  for (int k = 7; k >= 0; k--) c = c * y + cc[k];
  return c;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// unit quaternion (q[0]; q[1..3]) of the axis-angle vector v, through rotationCoefficients at
// y = (theta / 2)^2: sin(theta / 2) / theta = a(y) / 2, cos(theta / 2) = 1 - y b(y)
__device__ __forceinline__ void quaternionOf(const double* v, double* q) {
  const double y = 0.25 * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  double a, b, da, db;
  rotationCoefficients(y, a, b, da, db);
  q[0] = 1.0 - y * b;
#pragma unroll
  for (int i = 0; i < 3; i++) q[1 + i] = 0.5 * a * v[i];
}

// T <- exp(-step) T of one camera (BaAtLargeOptimizer.cpp:181-182, Sophus::SE3d::exp with the
// translation part first): d = -w, R' = exp([d]x) R(w_cam), t' = exp([d]x) t + V(d) (-u).  The rotations
// are composed as unit quaternions and brought back to an axis-angle vector of length <= pi by
// 2 atan2(|v|, q0) / |v|: no acos of a trace.
__device__ __forceinline__ void retractSe3(const double* cam, const double* stp, double* out) {
  const double d[3] = {-stp[3], -stp[4], -stp[5]}, u[3] = {-stp[0], -stp[1], -stp[2]};
  const double* t = cam + 3;
  // translation
  const double x = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  double a, b, da, db;
  rotationCoefficients(x, a, b, da, db);
  const double c = translationCoefficient(x);
  double dt[3], ddt[3], du[3], ddu[3];
  cross3(d, t, dt);
  cross3(d, dt, ddt);
  cross3(d, u, du);
  cross3(d, du, ddu);
#pragma unroll
  for (int i = 0; i < 3; i++) out[3 + i] = (t[i] + a * dt[i] + b * ddt[i]) + (u[i] + b * du[i] + c * ddu[i]);
  // rotation: q = q(d) * q(w_cam), normalised, q0 >= 0
  double p[4], r[4], q[4], pr[3];
  quaternionOf(d, p);
  quaternionOf(cam, r);
  cross3(p + 1, r + 1, pr);
  q[0] = p[0] * r[0] - (p[1] * r[1] + p[2] * r[2] + p[3] * r[3]);
#pragma unroll
  for (int i = 0; i < 3; i++) q[1 + i] = p[0] * r[1 + i] + r[0] * p[1 + i] + pr[i];
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sgn = q[0] < 0.0 ? -1.0 / nrm : 1.0 / nrm;
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] *= sgn;
  const double n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  double k;  // 2 atan2(|v|, q0) / |v|
  if (n2 < 1e-8) {  // q0 > 0.99: atan(z) / z = 1 - z^2 / 3 + z^4 / 5 - (z^6 / 7 < 2e-25), z = |v| / q0
    const double z2 = n2 / (q[0] * q[0]);
    k = 2.0 / q[0] * (1.0 + z2 * (-1.0 / 3 + z2 * (1.0 / 5)));
  } else {
    const double n = sqrt(n2);
    k = 2.0 * atan2(n, q[0]) / n;
  }
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = k * q[1 + i];
#pragma unroll
  for (int i = 6; i < 9; i++) out[i] = cam[i];
}

// Thread i < numPts retracts point i, thread numPts + c camera c; parameter p's slice of `step` starts
// at acc.paramStart(p) (points first, cameras after, as in balFillKernel).
template <bool SE3>
__global__ __launch_bounds__(256) void balApplyStepKernel(PermutedCoalescedAccessor acc, int64_t numPts,
                                                          int64_t numCams, const double* cams,
                                                          const double* pts, const double* step,
                                                          double* camsOut, double* ptsOut) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numPts + numCams) return;
  const double* stp = step + acc.paramStart(i);
  if (i < numPts) {
#pragma unroll
    for (int k = 0; k < 3; k++) ptsOut[3 * i + k] = pts[3 * i + k] - stp[k];
    return;
  }
  const double* cam = cams + 9 * (i - numPts);
  double* out = camsOut + 9 * (i - numPts);
  if (SE3) {
    retractSe3(cam, stp, out);
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = cam[k] - stp[k];
  }
}

}  // namespace

void balResiduals(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                  const double* cams, const double* pts, double* res, void* stream) {
  if (numObs <= 0) return;
  balResidualsKernel<<<dim3((unsigned)((numObs + 255) / 256)), 256, 0, (hipStream_t)stream>>>(
      numObs, obsCam, obsPt, obsXy, cams, pts, res);
  balCHECK(hipGetLastError());
}

void balResidualsSe3(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                     const double* cams, const double* pts, double* res, void* stream) {
  if (numObs <= 0) return;
  balResidualsSe3Kernel<<<dim3((unsigned)((numObs + 255) / 256)), 256, 0, (hipStream_t)stream>>>(
      numObs, obsCam, obsPt, obsXy, cams, pts, res);
  balCHECK(hipGetLastError());
}

void balLoss(int64_t numObs, int camSize, int kind, double a, double* res, double* Jc, double* Jp,
             double* rho, void* stream) {
  if (kind < 0 || kind > 2) {
    throw std::runtime_error("balLoss: unknown loss kind " + std::to_string(kind) +
                             " (0 trivial, 1 Huber, 2 Cauchy)");
  }
  if (!(a > 0.0) || !std::isfinite(a)) {
    throw std::runtime_error("balLoss: the loss size a must be finite and positive, got " + std::to_string(a));
  }
  if ((Jc == nullptr) != (Jp == nullptr)) {
    throw std::runtime_error("balLoss: Jc and Jp must both be given or both be NULL");
  }
  if (Jc != nullptr && camSize != 9 && camSize != 6) {
    throw std::runtime_error("balLoss: camera size must be 9 or 6");
  }
  if (numObs <= 0) return;
  const dim3 grid((unsigned)((numObs + kBalLossTile - 1) / kBalLossTile));
  if (camSize == 6) {
    balLossKernel<6><<<grid, kBalLossTile, 0, (hipStream_t)stream>>>(numObs, kind, a, res, Jc, Jp, rho);
  } else {
    balLossKernel<9><<<grid, kBalLossTile, 0, (hipStream_t)stream>>>(numObs, kind, a, res, Jc, Jp, rho);
  }
  balCHECK(hipGetLastError());
}

int64_t balSumScratchLen(int64_t n) { return n > 0 ? (n + kBalSumChunk - 1) / kBalSumChunk : 0; }

void balSum(int64_t n, const double* x, double scale, double* scratch, double* out, void* stream) {
  const int64_t nParts = balSumScratchLen(n);
  if (nParts > 0) {
    balSumPartial<<<dim3((unsigned)nParts), kBalSumWidth, 0, (hipStream_t)stream>>>(n, x, scratch);
  }
  balSumFinal<<<dim3(1), kBalSumWidth, 0, (hipStream_t)stream>>>(nParts, scratch, scale, out);
  balCHECK(hipGetLastError());
}

template <bool SE3>
static void launchApplyStep(const PermutedCoalescedAccessor& acc, int64_t numPts, int64_t numCams,
                            const double* cams, const double* pts, const double* step, double* camsOut,
                            double* ptsOut, void* stream) {
  const int64_t n = numPts + numCams;
  if (n <= 0) return;
  balApplyStepKernel<SE3><<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(
      acc, numPts, numCams, cams, pts, step, camsOut, ptsOut);
  balCHECK(hipGetLastError());
}

void balApplyStep(const PermutedCoalescedAccessor& acc, int64_t numPts, int64_t numCams, const double* cams,
                  const double* pts, const double* step, double* camsOut, double* ptsOut, void* stream) {
  launchApplyStep<false>(acc, numPts, numCams, cams, pts, step, camsOut, ptsOut, stream);
}

void balApplyStepSe3(const PermutedCoalescedAccessor& acc, int64_t numPts, int64_t numCams,
                     const double* cams, const double* pts, const double* step, double* camsOut,
                     double* ptsOut, void* stream) {
  launchApplyStep<true>(acc, numPts, numCams, cams, pts, step, camsOut, ptsOut, stream);
}

void balLinearize(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                  const double* cams, const double* pts, double* res, double* Jc, double* Jp,
                  void* stream) {
  if (numObs <= 0) return;
  balLinearizeKernel<<<dim3((unsigned)((numObs + 63) / 64)), 64, 0, (hipStream_t)stream>>>(
      numObs, obsCam, obsPt, obsXy, cams, pts, res, Jc, Jp);
  balCHECK(hipGetLastError());
}

void balLinearizeSe3(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* obsXy,
                     const double* cams, const double* pts, double* res, double* Jc, double* Jp,
                     void* stream) {
  if (numObs <= 0) return;
  balLinearizeSe3Kernel<<<dim3((unsigned)((numObs + 63) / 64)), 64, 0, (hipStream_t)stream>>>(
      numObs, obsCam, obsPt, obsXy, cams, pts, res, Jc, Jp);
  balCHECK(hipGetLastError());
}

template <typename T>
void balFillHessian(const PermutedCoalescedAccessor& acc, int camSize, int64_t numPts, int64_t numCams,
                    int64_t numObs, const int64_t* obsCam, const int64_t* obsPt, const double* Jc,
                    const double* Jp, const double* res, T lambda, T* data, T* grad, int64_t* dbg,
                    void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (numObs > 0) {
    balFillKernel<T><<<dim3((unsigned)((numObs + 3) / 4)), 256, 0, s>>>(
        acc, camSize, numPts, numCams, numObs, obsCam, obsPt, Jc, Jp, res, data, grad, dbg);
  }
  const int64_t numParams = numPts + numCams;
  if (lambda != T(0) && numParams > 0) {
    balDampKernel<T><<<dim3((unsigned)((numParams + 255) / 256)), 256, 0, s>>>(acc, numParams, lambda,
                                                                              data);
  }
  balCHECK(hipGetLastError());
}

template void balFillHessian<double>(const PermutedCoalescedAccessor&, int, int64_t, int64_t, int64_t,
                                     const int64_t*, const int64_t*, const double*, const double*,
                                     const double*, double, double*, double*, int64_t*, void*);
template void balFillHessian<float>(const PermutedCoalescedAccessor&, int, int64_t, int64_t, int64_t,
                                    const int64_t*, const int64_t*, const double*, const double*,
                                    const double*, float, float*, float*, int64_t*, void*);

// ---- ordered fill (bal_fill_plan.h, bal_fill_kernels.h) ------------------------------------------------
// The device copy of a plan: one allocation that holds every table the kernels read, each 16-byte
// aligned, and the scratch of the chunk partials behind them.
struct BalFillPlanDev {
  void* blob = nullptr;
  balfill::Tables tables;
  ~BalFillPlanDev() {
    if (blob) (void)hipFree(blob);
  }
};

void balFillPlanFreeDevice(BalFillPlanDev* dev) { delete dev; }

namespace {

struct BlobBuilder {
  std::vector<char> bytes;
  template <typename U>
  size_t add(const std::vector<U>& v) {
    const size_t at = (bytes.size() + 15) / 16 * 16;
    bytes.resize(at + v.size() * sizeof(U));
    if (!v.empty()) std::memcpy(bytes.data() + at, v.data(), v.size() * sizeof(U));
    return at;
  }
};

const balfill::Tables& uploadedTables(const BalFillPlan& m) {
  if (m.dev != nullptr) return m.dev->tables;
  BlobBuilder b;
  const size_t oPtPtr = b.add(m.ptPtr), oPtObs = b.add(m.ptObs), oPairPtr = b.add(m.pairPtr);
  const size_t oPairStride = b.add(m.pairStride), oPairFlip = b.add(m.pairFlip), oPairOff = b.add(m.pairOff);
  const size_t oCamObs = b.add(m.camObs), oCamChunkPtr = b.add(m.camChunkPtr), oChunkCam = b.add(m.chunkCam);
  const size_t oChunkBegin = b.add(m.chunkBegin), oChunkEnd = b.add(m.chunkEnd);
  const size_t oPtDiagOff = b.add(m.ptDiagOff), oCamDiagOff = b.add(m.camDiagOff), oPtStart = b.add(m.ptStart);
  const size_t oCamStart = b.add(m.camStart), oPtDiagStride = b.add(m.ptDiagStride);
  const size_t oCamDiagStride = b.add(m.camDiagStride);
  const size_t oPart = (b.bytes.size() + 15) / 16 * 16;
  std::unique_ptr<BalFillPlanDev> d(new BalFillPlanDev);
  balCHECK(hipMalloc(&d->blob, oPart + std::max<size_t>((size_t)m.scratchLen() * sizeof(double), 16)));
  if (!b.bytes.empty()) balCHECK(hipMemcpy(d->blob, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice));
  char* base = static_cast<char*>(d->blob);
  auto i32 = [base](size_t o) { return reinterpret_cast<const int32_t*>(base + o); };
  auto i64 = [base](size_t o) { return reinterpret_cast<const int64_t*>(base + o); };
  balfill::Tables& t = d->tables;
  t.ptPtr = i32(oPtPtr);
  t.ptObs = i32(oPtObs);
  t.pairPtr = i32(oPairPtr);
  t.pairStride = i32(oPairStride);
  t.pairFlip = i32(oPairFlip);
  t.pairOff = i64(oPairOff);
  t.camObs = i32(oCamObs);
  t.camChunkPtr = i32(oCamChunkPtr);
  t.chunkCam = i32(oChunkCam);
  t.chunkBegin = i32(oChunkBegin);
  t.chunkEnd = i32(oChunkEnd);
  t.ptDiagOff = i64(oPtDiagOff);
  t.camDiagOff = i64(oCamDiagOff);
  t.ptStart = i64(oPtStart);
  t.camStart = i64(oCamStart);
  t.ptDiagStride = i32(oPtDiagStride);
  t.camDiagStride = i32(oCamDiagStride);
  t.part = reinterpret_cast<double*>(base + oPart);
  m.dev = d.release();
  return m.dev->tables;
}

unsigned gridFor(int64_t threads) { return (unsigned)((threads + balfill::kThreads - 1) / balfill::kThreads); }

template <typename T, int CS>
void launchFillOrdered(const BalFillPlan& m, const balfill::Tables& t, const double* Jc, const double* Jp,
                       const double* res, T* data, T* grad, hipStream_t s) {
  using namespace balfill;
  if (m.numPairs() > 0) {
    balFillPairs<T, CS><<<dim3(gridFor(m.numPairs() * 3 * CS)), kThreads, 0, s>>>(m.numPairs(), t, Jc, Jp, data);
  }
  if (m.numKept > 0) {
    balFillPoints<T><<<dim3(gridFor(m.numPts * 12)), kThreads, 0, s>>>(m.numPts, t, Jp, res, data, grad);
    balFillCamChunks<CS><<<dim3((unsigned)m.numChunks()), kThreads, 0, s>>>(t, Jc, res);
    balFillCamFold<T, CS><<<dim3(gridFor(m.numCams * Partial<CS>::kWords)), kThreads, 0, s>>>(m.numCams, t, data,
                                                                                             grad);
  }
}

}  // namespace

template <typename T>
void balFillOrdered(const BalFillPlan& plan, const double* Jc, const double* Jp, const double* res, T lambda,
                    T* data, T* grad, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (plan.numKept > 0) {
    const balfill::Tables& t = uploadedTables(plan);
    if (plan.camSize == 6) {
      launchFillOrdered<T, 6>(plan, t, Jc, Jp, res, data, grad, s);
    } else {
      launchFillOrdered<T, 9>(plan, t, Jc, Jp, res, data, grad, s);
    }
  }
  const int64_t numParams = plan.numPts + plan.numCams;
  if (lambda != T(0) && numParams > 0) {
    balDampKernel<T><<<dim3((unsigned)((numParams + 255) / 256)), 256, 0, s>>>(plan.solver->deviceAccessor(),
                                                                              numParams, lambda, data);
  }
  balCHECK(hipGetLastError());
}

template void balFillOrdered<double>(const BalFillPlan&, const double*, const double*, const double*, double,
                                     double*, double*, void*);
template void balFillOrdered<float>(const BalFillPlan&, const double*, const double*, const double*, float, float*,
                                    float*, void*);

}  // namespace BaSpaCho
