// Device code shared by the multi-view geometry translation units (geometry.hip, pseudo_label.hip):
// pymvg's undistortion and projection restated, the DLT point of a row set, and the per-(group,
// joint) view loader of the pseudo-label kernels.  Everything is fp64 and lives in registers when
// the view indices are compile-time.
#pragma once
#include "posu_common.h"

namespace posu {

// pymvg CameraModel.undistort (OpenCV fixed point, 5 iterations); returns the input
// unchanged when every coefficient is zero, as pymvg does
__device__ __forceinline__ void undistort_px(const double* c, double& u, double& v) {
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
  const double k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8];
  if (fabs(k1) + fabs(k2) + fabs(p1) + fabs(p2) + fabs(k3) == 0.0) return;
  const double xd = (u - cx) / fx, yd = (v - cy) / fy;
  double xx = xd, yy = yd;
#pragma unroll
  for (int it = 0; it < 5; ++it) {
    const double r2 = xx * xx + yy * yy;
    const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
    const double dX = 2.0 * p1 * xx * yy + p2 * (r2 + 2.0 * xx * xx);
    const double dY = p1 * (r2 + 2.0 * yy * yy) + 2.0 * p2 * xx * yy;
    xx = (xd - dX) * icdist;
    yy = (yd - dY) * icdist;
  }
  u = xx * fx + cx;
  v = yy * fy + cy;
}

// Smallest right singular vector of A (one-sided Jacobi), dehomogenised: the DLT
// point of pymvg MultiCameraSystem.find3d (svd -> vt[-1, :3] / vt[-1, 3]).
template <int ROWS>
__device__ __forceinline__ void dlt_point(double (&A)[ROWS][4], double* out) {
  // rotate column pairs of A until mutually orthogonal; Vm accumulates the rotations
  double Vm[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          alpha += A[r][p] * A[r][p];
          beta += A[r][q] * A[r][q];
          gamma += A[r][p] * A[r][q];
        }
        if (gamma != 0.0 && fabs(gamma) > 1e-15 * sqrt(alpha * beta)) {
          rotated = true;
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            const double ap = A[r][p], aq = A[r][q];
            A[r][p] = cs * ap - sn * aq;
            A[r][q] = sn * ap + cs * aq;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double vp = Vm[r][p], vq = Vm[r][q];
            Vm[r][p] = cs * vp - sn * vq;
            Vm[r][q] = sn * vp + cs * vq;
          }
        }
      }
    }
    if (!rotated) break;
  }
  double nrm[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    nrm[c] = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) nrm[c] += A[r][c] * A[r][c];
  }
  double v0 = Vm[0][0], v1 = Vm[1][0], v2 = Vm[2][0], v3 = Vm[3][0], bn = nrm[0];
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    if (nrm[c] < bn) {
      bn = nrm[c];
      v0 = Vm[0][c];
      v1 = Vm[1][c];
      v2 = Vm[2][c];
      v3 = Vm[3][c];
    }
  }
  out[0] = v0 / v3;
  out[1] = v1 / v3;
  out[2] = v2 / v3;
}

constexpr int kPairViews = 4;

__device__ __forceinline__ void project_px(const double* M, const double* c, const double* X, double& u, double& v) {
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
  const double k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8];
  // [R|t] = K^-1 M (zero-skew K)
  double P[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) P[r] = M[4 * r] * X[0] + M[4 * r + 1] * X[1] + M[4 * r + 2] * X[2] + M[4 * r + 3];
  const double zc = P[2];
  const double yc = (P[1] - cy * P[2]) / fy;
  const double xc = (P[0] - cx * P[2]) / fx;
  const double x = xc / zc, y = yc / zc;
  const double r2 = x * x + y * y;
  const double radial = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
  const double yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
  u = fx * xd + cx;
  v = fy * yd + cy;
}

struct ViewPts {
  double raw[kPairViews][2];  // predictions as given (reprojection errors are measured on these)
  double und[kPairViews][2];  // undistorted (the DLT rows)
  bool on[kPairViews];
  int nvis;
};

__device__ __forceinline__ void load_views(const double* Mall, const double* intr, const double* xy,
                                           const unsigned char* vis, int g, int k, int V, int J, int undistort,
                                           ViewPts& p) {
  p.nvis = 0;
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    const size_t gv = static_cast<size_t>(g) * V + (v < V ? v : 0);
    p.on[v] = v < V && (!vis || vis[gv * J + k]);
    const double* q = xy + (gv * J + k) * 2;
    p.raw[v][0] = v < V ? q[0] : 0.0;
    p.raw[v][1] = v < V ? q[1] : 0.0;
    double u = p.raw[v][0], w = p.raw[v][1];
    if (p.on[v] && undistort) undistort_px(intr + gv * 9, u, w);
    p.und[v][0] = u;
    p.und[v][1] = w;
    if (p.on[v]) ++p.nvis;
  }
}

}  // namespace posu
