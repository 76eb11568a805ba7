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

// ------------------------------------------------------------------------------------------------------------
// The differentiable triangulation (triangulate_grad.hip).  These stand beside the functions above, whose
// arithmetic they leave alone: the derivative of undistort_px, the reverse of project_px, a loader that also
// takes f32 / strided predictions and row weights, and the weighted DLT solve with everything its reverse needs.

// undistort_px with D = d(u, v)_out / d(u, v)_in of the function as it is computed: the tangents of the five
// fixed-point iterations are carried beside them.  (The implicit-function derivative would be that of the limit,
// not of the fifth iterate.)  The identity when every coefficient is zero, like the function.
__device__ __forceinline__ void undistort_px_jac(const double* c, double& u, double& v, double (&D)[2][2]) {
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
  const double k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8];
  D[0][0] = D[1][1] = 1.0;
  D[0][1] = D[1][0] = 0.0;
  if (fabs(k1) + fabs(k2) + fabs(p1) + fabs(p2) + fabs(k3) == 0.0) return;
  const double xd = (u - cx) / fx, yd = (v - cy) / fy;
  double xx = xd, yy = yd;
  double xa = 1.0, xb = 0.0, ya = 0.0, yb = 1.0;  // d xx / d xd, d xx / d yd, d yy / d xd, d yy / d yd
#pragma unroll
  for (int it = 0; it < 5; ++it) {
    const double r2 = xx * xx + yy * yy;
    const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
    const double dX = 2.0 * p1 * xx * yy + p2 * (r2 + 2.0 * xx * xx);
    const double dY = p1 * (r2 + 2.0 * yy * yy) + 2.0 * p2 * xx * yy;
    const double dpoly = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1;  // d (1 / icdist) / d r2
    const double r2a = 2.0 * (xx * xa + yy * ya), r2b = 2.0 * (xx * xb + yy * yb);
    const double ica = -icdist * icdist * dpoly * r2a, icb = -icdist * icdist * dpoly * r2b;
    const double xya = xa * yy + xx * ya, xyb = xb * yy + xx * yb;  // d (xx yy)
    const double dXa = 2.0 * p1 * xya + p2 * (r2a + 4.0 * xx * xa), dXb = 2.0 * p1 * xyb + p2 * (r2b + 4.0 * xx * xb);
    const double dYa = p1 * (r2a + 4.0 * yy * ya) + 2.0 * p2 * xya, dYb = p1 * (r2b + 4.0 * yy * yb) + 2.0 * p2 * xyb;
    const double nx = xd - dX, ny = yd - dY;
    xa = (1.0 - dXa) * icdist + nx * ica;
    xb = -dXb * icdist + nx * icb;
    ya = -dYa * icdist + ny * ica;
    yb = (1.0 - dYb) * icdist + ny * icb;
    xx = nx * icdist;
    yy = ny * icdist;
  }
  u = xx * fx + cx;
  v = yy * fy + cy;
  D[0][0] = xa;
  D[0][1] = xb * fx / fy;
  D[1][0] = ya * fy / fx;
  D[1][1] = yb;
}

// The reverse of project_px in X: gX += J^T (gu, gv) with J = d(u, v) / dX at X
__device__ __forceinline__ void project_px_vjp(const double* M, const double* c, const double* X, double gu, double gv,
                                               double (&gX)[3]) {
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
  const double k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8];
  double P[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) P[r] = M[4 * r] * X[0] + M[4 * r + 1] * X[1] + M[4 * r + 2] * X[2] + M[4 * r + 3];
  const double zc = P[2];
  const double x = (P[0] - cx * P[2]) / fx / zc, y = (P[1] - cy * P[2]) / fy / zc;
  const double r2 = x * x + y * y;
  const double radial = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double drad = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1;  // d radial / d r2
  const double gxd = fx * gu, gyd = fy * gv;
  const double gx = gxd * (radial + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x) +
                    gyd * (2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y);
  const double gy = gxd * (2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y) +
                    gyd * (radial + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x);
  const double gxc = gx / zc, gyc = gy / zc;
  const double gP0 = gxc / fx, gP1 = gyc / fy;
  const double gP2 = -(gx * x + gy * y) / zc - cx * gP0 - cy * gP1;
#pragma unroll
  for (int j = 0; j < 3; ++j) gX[j] += gP0 * M[j] + gP1 * M[4 + j] + gP2 * M[8 + j];
}

// ViewPts for the differentiable kernels: predictions in f32 or f64 at xy[g * sg + v * sv + 2 k] (the layouts of
// posu_triangulate_dlt), the Jacobian of each view's undistortion, and the DLT row weight (1 without a table)
struct ViewPtsGrad {
  double raw[kPairViews][2];
  double und[kPairViews][2];
  double D[kPairViews][2][2];  // d und / d raw
  double w[kPairViews];
  bool on[kPairViews];
  int nvis;
};

__device__ __forceinline__ void load_views_grad(const double* intr, const void* xyv, int xy_dtype, int sg, int sv,
                                                const unsigned char* vis, const double* w, int g, int k, int V, int J,
                                                int undistort, ViewPtsGrad& p) {
  p.nvis = 0;
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    const size_t gv = static_cast<size_t>(g) * V + (v < V ? v : 0);
    p.on[v] = v < V && (!vis || vis[gv * J + k]);
    const size_t xoff = static_cast<size_t>(g) * sg + static_cast<size_t>(v < V ? v : 0) * sv + 2 * k;
    double u, y;
    if (xy_dtype == POSU_F64) {
      u = static_cast<const double*>(xyv)[xoff];
      y = static_cast<const double*>(xyv)[xoff + 1];
    } else {
      u = static_cast<const float*>(xyv)[xoff];
      y = static_cast<const float*>(xyv)[xoff + 1];
    }
    p.raw[v][0] = v < V ? u : 0.0;
    p.raw[v][1] = v < V ? y : 0.0;
    p.D[v][0][0] = p.D[v][1][1] = 1.0;
    p.D[v][0][1] = p.D[v][1][0] = 0.0;
    if (p.on[v] && undistort) undistort_px_jac(intr + gv * 9, u, y, p.D[v]);
    p.und[v][0] = u;
    p.und[v][1] = y;
    p.w[v] = (p.on[v] && w) ? w[gv * J + k] : 1.0;
    if (p.on[v]) ++p.nvis;
  }
}

// The weighted DLT solve: A's rows of view v are w_v (u m2 - m0), w_v (v m2 - m1), zero for a view that is off.
// Kept for the reverse: Q's columns q_i (the right singular vectors), lam_i = sigma_i^2, AQ = A Q (column i is
// A q_i: what jacobi_columns leaves in A), and the smallest one's index, chosen as dlt_point chooses it.
struct DltSolve {
  double AQ[2 * kPairViews][4];
  double Q[4][4];
  double lam[4];
  double h[4];  // q_min
  double X[3];  // h[:3] / h[3]
  int imin;
};

__device__ __forceinline__ void dlt_solve_w(const double* Mall, const ViewPtsGrad& p, int g, int V, DltSolve& s) {
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    dlt_rows(Mall + (static_cast<size_t>(g) * V + (v < V ? v : 0)) * 12, p.und[v][0], p.und[v][1], p.on[v],
             s.AQ[2 * v], s.AQ[2 * v + 1]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s.AQ[2 * v][c] *= p.w[v];
      s.AQ[2 * v + 1][c] *= p.w[v];
    }
  }
  jacobi_columns<2 * kPairViews, 4>(s.AQ, s.Q);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    s.lam[c] = 0;
#pragma unroll
    for (int r = 0; r < 2 * kPairViews; ++r) s.lam[c] += s.AQ[r][c] * s.AQ[r][c];
  }
  s.imin = 0;
  double bn = s.lam[0];
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    if (s.lam[c] < bn) {
      bn = s.lam[c];
      s.imin = c;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    s.h[r] = s.Q[r][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) s.h[r] = s.imin == c ? s.Q[r][c] : s.h[r];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) s.X[r] = s.h[r] / s.h[3];
}

// The reverse of the solve.  With B = A^T A = sum lam_i q_i q_i^T, h = q_min and X = h[:3] / h[3]:
//   gh = (gX / h3, -(gX . X) / h3),   z = sum_{i != min} q_i (q_i . gh) / (lam_min - lam_i),
//   gA = (A z) h^T + (A h) z^T.
// A row a = w (u m2 - m0) then gives g_u = w (gA_row . m2) and g_w += gA_row . (u m2 - m0); gA is never formed:
// row r of it is (A z)_r h + (A h)_r z, and A z, A h come from the columns of AQ.  A repeated smallest eigenvalue
// (a degenerate rig) drops its term instead of dividing by zero.
// gund[v]: d / d und of view v (zero for a view that is off); gw[v]: d / d w_v.
__device__ __forceinline__ void dlt_solve_vjp(const double* Mall, const ViewPtsGrad& p, int g, int V,
                                              const DltSolve& s, const double (&gX)[3],
                                              double (&gund)[kPairViews][2], double (&gw)[kPairViews]) {
  const double h3 = s.h[3];
  const double gh[4] = {gX[0] / h3, gX[1] / h3, gX[2] / h3,
                        -(gX[0] * s.X[0] + gX[1] * s.X[1] + gX[2] * s.X[2]) / h3};
  double lmin = s.lam[0];
#pragma unroll
  for (int c = 1; c < 4; ++c) lmin = s.imin == c ? s.lam[c] : lmin;
  double coef[4], z[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double d = lmin - s.lam[i];
    const double dot = s.Q[0][i] * gh[0] + s.Q[1][i] * gh[1] + s.Q[2][i] * gh[2] + s.Q[3][i] * gh[3];
    coef[i] = (s.imin == i || d == 0.0) ? 0.0 : dot / d;
#pragma unroll
    for (int r = 0; r < 4; ++r) z[r] += s.Q[r][i] * coef[i];
  }
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    gund[v][0] = gund[v][1] = 0.0;
    gw[v] = 0.0;
    if (!p.on[v]) continue;
    const double* M = Mall + (static_cast<size_t>(g) * V + v) * 12;
    const double hm2 = s.h[0] * M[8] + s.h[1] * M[9] + s.h[2] * M[10] + s.h[3] * M[11];
    const double zm2 = z[0] * M[8] + z[1] * M[9] + z[2] * M[10] + z[3] * M[11];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int r = 2 * v + e;
      double Az = 0.0, Ah = s.AQ[r][0];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Az += s.AQ[r][i] * coef[i];
        Ah = s.imin == i ? s.AQ[r][i] : Ah;
      }
      const double* Me = M + 4 * e;
      const double hme = s.h[0] * Me[0] + s.h[1] * Me[1] + s.h[2] * Me[2] + s.h[3] * Me[3];
      const double zme = z[0] * Me[0] + z[1] * Me[1] + z[2] * Me[2] + z[3] * Me[3];
      gund[v][e] = p.w[v] * (Az * hm2 + Ah * zm2);
      gw[v] += Az * (p.und[v][e] * hm2 - hme) + Ah * (p.und[v][e] * zm2 - zme);
    }
  }
}

}  // namespace posu
