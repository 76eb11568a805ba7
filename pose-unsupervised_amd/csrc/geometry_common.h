// The one home of the fp64 small-matrix and view arithmetic (geometry.hip, pseudo_label.hip,
// pose3d.hip): the Hestenes Jacobi loop, pymvg's undistortion and projection restated, the DLT rows
// and point, the per-(group, joint) view loader, and the pair hypothesis / n-view re-projection of the
// pseudo-label kernels.  Everything lives in registers when the view indices are compile-time.
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

// One-sided (Hestenes) Jacobi: column pairs of A are rotated until mutually orthogonal and V (set to
// the identity here) accumulates the rotations, so that on return A = U diag(s) and V holds the right
// singular vectors: column c's norm is s_c.  At most 30 sweeps.  Every index is a compile-time
// constant, so both matrices live in registers.
// The loop runs on private copies.  Behind reference parameters the two arrays may alias for all the
// compiler knows while it optimises this function on its own, before it inlines it; that form rounded
// some sums differently from the loop written out in its callers and took 8 to 28 more VGPRs per kernel.
// That is a property of one compiler: after a ROCm upgrade run tools/pseudo_label_micro.py --digest and
// tools/pose3d_micro.py --digest and compare with profiles/r12/geometry_refactor_digest.txt.
template <int ROWS, int N>
__device__ __forceinline__ void jacobi_columns(double (&A_io)[ROWS][N], double (&V_out)[N][N]) {
  double A[ROWS][N], V[N][N];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) A[r][c] = A_io[r][c];
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          alpha += A[r][p] * A[r][p];
          beta += A[r][q] * A[r][q];
          gamma += A[r][p] * A[r][q];
        }
        // false for NaN: a degenerate input (0 / 0 upstream) stops rotating at once instead of spinning
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
          for (int r = 0; r < N; ++r) {
            const double vp = V[r][p], vq = V[r][q];
            V[r][p] = cs * vp - sn * vq;
            V[r][q] = sn * vp + cs * vq;
          }
        }
      }
    }
    if (!rotated) break;
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) A_io[r][c] = A[r][c];
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) V_out[r][c] = V[r][c];
}

// Smallest right singular vector of A, dehomogenised: the DLT point of pymvg
// MultiCameraSystem.find3d (svd -> vt[-1, :3] / vt[-1, 3]).
template <int ROWS>
__device__ __forceinline__ void dlt_point(double (&A)[ROWS][4], double* out) {
  double Vm[4][4];
  jacobi_columns<ROWS, 4>(A, Vm);
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

// The two DLT rows of a view with projection matrix M (3 x 4, row major) that saw the undistorted
// pixel (u, v); zero rows for a view that is not on (they add nothing to A^T A).
__device__ __forceinline__ void dlt_rows(const double* M, double u, double v, bool on, double (&row0)[4],
                                         double (&row1)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    row0[c] = on ? u * M[8 + c] - M[c] : 0.0;
    row1[c] = on ? v * M[8 + c] - M[4 + c] : 0.0;
  }
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

// The functions below take their view indices (a, b, the loop counters) as compile-time constants
// once they are inlined into unrolled loops, so ViewPts' arrays stay in registers -- a run-time
// index put them in 144 B of scratch.

// One RANSAC hypothesis (triangulate.py:102-165): views a and b triangulated, the point projected
// into the V views; the views within thre of their prediction, their number and their error sum.
struct PairScore {
  int mask, n;
  double err_sum;
};

__device__ __forceinline__ PairScore score_pair(const double* Mall, const double* intr, const ViewPts& p, int g,
                                                int V, int a, int b, double thre) {
  double A[4][4];
  dlt_rows(Mall + (static_cast<size_t>(g) * V + a) * 12, p.und[a][0], p.und[a][1], true, A[0], A[1]);
  dlt_rows(Mall + (static_cast<size_t>(g) * V + b) * 12, p.und[b][0], p.und[b][1], true, A[2], A[3]);
  double X[3];
  dlt_point<4>(A, X);
  PairScore s = {0, 0, 0.0};
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    if (v >= V) break;
    const size_t gv = static_cast<size_t>(g) * V + v;
    double u, w;
    project_px(Mall + gv * 12, intr + gv * 9, X, u, w);
    const double du = u - p.raw[v][0], dv = w - p.raw[v][1];
    const double e = sqrt(du * du + dv * dv);
    if (e < thre) {
      s.mask |= 1 << v;
      ++s.n;
      s.err_sum += e;
    }
  }
  return s;
}

// The hypothesis RANSAC keeps: more inliers, then the smaller mean inlier error
struct BestPair {
  int mask = 0, n = 0;
  double err = 10000.0;
  __device__ __forceinline__ void offer(int pair_mask, int pair_n, double pair_err) {
    if (pair_n > n || (pair_n == n && pair_err < err)) {
      n = pair_n;
      mask = pair_mask;
      err = pair_err;
    }
  }
};

// reproject_poses (triangulate.py:169-213): the DLT point of the views in mask, projected into the V views
__device__ __forceinline__ void solve_project(const double* Mall, const double* intr, const ViewPts& p, int g, int V,
                                              int mask, double (&pj)[kPairViews][2]) {
  double A[2 * kPairViews][4];
#pragma unroll
  for (int v = 0; v < kPairViews; ++v)
    dlt_rows(Mall + (static_cast<size_t>(g) * V + (v < V ? v : 0)) * 12, p.und[v][0], p.und[v][1], (mask >> v) & 1,
             A[2 * v], A[2 * v + 1]);
  double X[3];
  dlt_point<2 * kPairViews>(A, X);
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    if (v >= V) break;
    const size_t gv = static_cast<size_t>(g) * V + v;
    project_px(Mall + gv * 12, intr + gv * 9, X, pj[v][0], pj[v][1]);
  }
}

}  // namespace posu
