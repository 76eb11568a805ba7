// Differentiable n-view triangulation and the reprojection-consistency loss built on it (2 <= V <= 4).
//
// One thread per (group, joint), all fp64, every view index a compile-time constant (geometry_common.h says
// what a run-time index costs).  The forward is posu_triangulate_dlt's with a weight per view on the two DLT
// rows; the backward recomputes it and goes back through the smallest right singular vector (dlt_solve_vjp),
// the DLT rows and the five undistortion iterations (undistort_px_jac).  The loss triangulates the predictions
// of all views, projects the point into every view with the lens model (project_px) and averages the pixel
// distance to the predictions:
//   loss = sum_{g, v, k} omega[g][v][k] ||project_v(X[g][k]) - xy[g][v][k]|| / (G V J).
// Its backward sends the gradient into the predictions directly and, unless the point is detached, through X.
//
// No atomics, no allocation: each 256-thread block of the loss sums its threads in a fixed order (wave_sum, then
// the four waves) into one workspace slot, and a second one-block launch sums the slots in a fixed order, so the
// same inputs give the same bits.  Every output element is written by exactly one thread.
#include "geometry_common.h"
#include "posu_common.h"

namespace posu {
namespace {

constexpr int kLossBlock = 256;

__device__ __forceinline__ void store_xy(void* out, int xy_dtype, size_t off, double a, double b) {
  if (xy_dtype == POSU_F64) {
    static_cast<double*>(out)[off] = a;
    static_cast<double*>(out)[off + 1] = b;
  } else {
    static_cast<float*>(out)[off] = static_cast<float>(a);
    static_cast<float*>(out)[off + 1] = static_cast<float>(b);
  }
}

__device__ __forceinline__ size_t xy_offset(int g, int v, int k, int sg, int sv) {
  return static_cast<size_t>(g) * sg + static_cast<size_t>(v) * sv + 2 * k;
}

__global__ __launch_bounds__(64) void triangulate_w_kernel(const double* __restrict__ Mall,
                                                           const double* __restrict__ intr,
                                                           const void* __restrict__ xyv, int xy_dtype, int sg, int sv,
                                                           const unsigned char* __restrict__ vis,
                                                           const double* __restrict__ w, int G, int V, int J,
                                                           int undistort, double* __restrict__ X) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= G * J) return;
  const int g = t / J, k = t - g * J;
  ViewPtsGrad p;
  load_views_grad(intr, xyv, xy_dtype, sg, sv, vis, w, g, k, V, J, undistort, p);
  double* out = X + static_cast<size_t>(t) * 3;
  if (p.nvis < 2) {
    out[0] = out[1] = out[2] = 0.0;
    return;
  }
  DltSolve s;
  dlt_solve_w(Mall, p, g, V, s);
  out[0] = s.X[0];
  out[1] = s.X[1];
  out[2] = s.X[2];
}

// raw-pixel gradient of a view from the gradient at its undistorted pixel: D^T gund
__device__ __forceinline__ void through_undistort(const ViewPtsGrad& p, int v, const double (&gund)[kPairViews][2],
                                                  double& gu, double& gv) {
  gu = p.D[v][0][0] * gund[v][0] + p.D[v][1][0] * gund[v][1];
  gv = p.D[v][0][1] * gund[v][0] + p.D[v][1][1] * gund[v][1];
}

__global__ __launch_bounds__(64) void triangulate_bwd_kernel(const double* __restrict__ Mall,
                                                             const double* __restrict__ intr,
                                                             const void* __restrict__ xyv, int xy_dtype, int sg,
                                                             int sv, const unsigned char* __restrict__ vis,
                                                             const double* __restrict__ w, int G, int V, int J,
                                                             int undistort, const double* __restrict__ gXall,
                                                             void* __restrict__ gxy, double* __restrict__ gwout) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= G * J) return;
  const int g = t / J, k = t - g * J;
  ViewPtsGrad p;
  load_views_grad(intr, xyv, xy_dtype, sg, sv, vis, w, g, k, V, J, undistort, p);
  double gund[kPairViews][2], gw[kPairViews];
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) gund[v][0] = gund[v][1] = gw[v] = 0.0;
  if (p.nvis >= 2) {
    DltSolve s;
    dlt_solve_w(Mall, p, g, V, s);
    const double gX[3] = {gXall[static_cast<size_t>(t) * 3], gXall[static_cast<size_t>(t) * 3 + 1],
                          gXall[static_cast<size_t>(t) * 3 + 2]};
    dlt_solve_vjp(Mall, p, g, V, s, gX, gund, gw);
  }
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    if (v >= V) break;
    double gu, gv;
    through_undistort(p, v, gund, gu, gv);
    store_xy(gxy, xy_dtype, xy_offset(g, v, k, sg, sv), gu, gv);
    if (gwout) gwout[(static_cast<size_t>(g) * V + v) * J + k] = gw[v];
  }
}

// residual weight of view v: the table's (1 without one), 0 for a view that is off or a joint that was not solved
__device__ __forceinline__ double residual_weight(const double* omega, const ViewPtsGrad& p, int v, bool solved,
                                                  size_t idx) {
  if (!solved || !p.on[v]) return 0.0;
  return omega ? omega[idx] : 1.0;
}

__global__ __launch_bounds__(kLossBlock) void reprojection_fwd_kernel(
    const double* __restrict__ Mall, const double* __restrict__ intr, const void* __restrict__ xyv, int xy_dtype,
    int sg, int sv, const unsigned char* __restrict__ vis, const double* __restrict__ w,
    const double* __restrict__ omega, int G, int V, int J, int undistort, double* __restrict__ part,
    double* __restrict__ Xout, double* __restrict__ eout) {
  const int t = blockIdx.x * kLossBlock + threadIdx.x;
  double acc = 0.0;
  if (t < G * J) {
    const int g = t / J, k = t - g * J;
    ViewPtsGrad p;
    load_views_grad(intr, xyv, xy_dtype, sg, sv, vis, w, g, k, V, J, undistort, p);
    const bool solved = p.nvis >= 2;
    double X[3] = {0.0, 0.0, 0.0};
    if (solved) {
      DltSolve s;
      dlt_solve_w(Mall, p, g, V, s);
      X[0] = s.X[0];
      X[1] = s.X[1];
      X[2] = s.X[2];
    }
#pragma unroll
    for (int v = 0; v < kPairViews; ++v) {
      if (v >= V) break;
      const size_t gv = static_cast<size_t>(g) * V + v;
      double e = 0.0;
      if (solved) {
        double u, y;
        project_px(Mall + gv * 12, intr + gv * 9, X, u, y);
        const double du = u - p.raw[v][0], dv = y - p.raw[v][1];
        e = sqrt(du * du + dv * dv);
      }
      const double om = residual_weight(omega, p, v, solved, gv * J + k);
      if (om != 0.0) acc += om * e;
      if (eout) eout[gv * J + k] = e;
    }
    if (Xout) {
      Xout[static_cast<size_t>(t) * 3] = X[0];
      Xout[static_cast<size_t>(t) * 3 + 1] = X[1];
      Xout[static_cast<size_t>(t) * 3 + 2] = X[2];
    }
  }
  __shared__ double wave_part[kLossBlock / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(kLossBlock) void reprojection_sum_kernel(const double* __restrict__ part, int nparts,
                                                                     double divisor, double* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kLossBlock) acc += part[i];
  __shared__ double wave_part[kLossBlock / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = ((wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3])) / divisor;
}

__global__ __launch_bounds__(64) void reprojection_bwd_kernel(
    const double* __restrict__ Mall, const double* __restrict__ intr, const void* __restrict__ xyv, int xy_dtype,
    int sg, int sv, const unsigned char* __restrict__ vis, const double* __restrict__ w,
    const double* __restrict__ omega, int G, int V, int J, int undistort, int detach_point,
    const double* __restrict__ gloss, void* __restrict__ gxy, double* __restrict__ gwout) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= G * J) return;
  const int g = t / J, k = t - g * J;
  ViewPtsGrad p;
  load_views_grad(intr, xyv, xy_dtype, sg, sv, vis, w, g, k, V, J, undistort, p);
  const double gl = gloss[0] / (static_cast<double>(G) * V * J);
  double graw[kPairViews][2], gund[kPairViews][2], gw[kPairViews];
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) graw[v][0] = graw[v][1] = gund[v][0] = gund[v][1] = gw[v] = 0.0;
  if (p.nvis >= 2) {
    DltSolve s;
    dlt_solve_w(Mall, p, g, V, s);
    double gX[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < kPairViews; ++v) {
      if (v >= V) break;
      const size_t gv = static_cast<size_t>(g) * V + v;
      const double om = residual_weight(omega, p, v, true, gv * J + k);
      if (om == 0.0) continue;
      double u, y;
      project_px(Mall + gv * 12, intr + gv * 9, s.X, u, y);
      const double du = u - p.raw[v][0], dv = y - p.raw[v][1];
      const double e = sqrt(du * du + dv * dv);
      if (!(e > 0.0)) continue;  // r = 0: the subgradient 0, never 0 / 0
      const double cu = gl * om * du / e, cv = gl * om * dv / e;
      graw[v][0] = -cu;
      graw[v][1] = -cv;
      if (!detach_point) project_px_vjp(Mall + gv * 12, intr + gv * 9, s.X, cu, cv, gX);
    }
    if (!detach_point) dlt_solve_vjp(Mall, p, g, V, s, gX, gund, gw);
  }
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) {
    if (v >= V) break;
    double gu, gv;
    through_undistort(p, v, gund, gu, gv);
    store_xy(gxy, xy_dtype, xy_offset(g, v, k, sg, sv), graw[v][0] + gu, graw[v][1] + gv);
    if (gwout) gwout[(static_cast<size_t>(g) * V + v) * J + k] = gw[v];
  }
}

}  // namespace
}  // namespace posu

using namespace posu;

// the checks every entry point here shares; the name goes in front of the message
#define POSU_REQUIRE_TRI(name)                                                                                  \
  POSU_REQUIRE(G >= 0 && V >= 2 && V <= kPairViews && J > 0, name ": bad shape (2 <= V <= 4)");                 \
  POSU_REQUIRE(static_cast<long long>(G) * J <= (1LL << 28), name ": bad shape (G * J <= 2^28)");               \
  POSU_REQUIRE(xy_dtype == POSU_F32 || xy_dtype == POSU_F64, name ": xy dtype must be F32 or F64");             \
  POSU_REQUIRE(xy_stride_g >= 0 && xy_stride_v >= 0, name ": negative xy stride")

extern "C" int posu_triangulate_dlt_w(const double* M, const double* intr, const void* xy, int xy_dtype,
                                      int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                                      int G, int V, int J, int undistort, double* X, void* stream) {
  POSU_REQUIRE(M && intr && xy && X, "posu_triangulate_dlt_w: null pointer");
  POSU_REQUIRE_TRI("posu_triangulate_dlt_w");
  // without weights this IS posu_triangulate_dlt: the same kernel, so the same bits
  if (!w) return posu_triangulate_dlt(M, intr, xy, xy_dtype, xy_stride_g, xy_stride_v, vis, G, V, J, undistort, X, stream);
  if (G == 0) return POSU_OK;
  hipLaunchKernelGGL(triangulate_w_kernel, dim3((G * J + 63) / 64), dim3(64), 0, as_stream(stream), M, intr, xy,
                     xy_dtype, xy_stride_g, xy_stride_v, vis, w, G, V, J, undistort, X);
  return check_launch("posu_triangulate_dlt_w");
}

extern "C" int posu_triangulate_dlt_bwd(const double* M, const double* intr, const void* xy, int xy_dtype,
                                        int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                                        int G, int V, int J, int undistort, const double* gX, void* gxy, double* gw,
                                        void* stream) {
  POSU_REQUIRE(M && intr && xy && gX && gxy, "posu_triangulate_dlt_bwd: null pointer");
  POSU_REQUIRE_TRI("posu_triangulate_dlt_bwd");
  if (G == 0) return POSU_OK;
  hipLaunchKernelGGL(triangulate_bwd_kernel, dim3((G * J + 63) / 64), dim3(64), 0, as_stream(stream), M, intr, xy,
                     xy_dtype, xy_stride_g, xy_stride_v, vis, w, G, V, J, undistort, gX, gxy, gw);
  return check_launch("posu_triangulate_dlt_bwd");
}

extern "C" long long posu_reprojection_loss_workspace(int G, int J) {
  if (G < 0 || J <= 0 || static_cast<long long>(G) * J > (1LL << 28)) return -1;
  const long long blocks = (static_cast<long long>(G) * J + kLossBlock - 1) / kLossBlock;
  return std::max(blocks, 1LL) * static_cast<long long>(sizeof(double));
}

extern "C" int posu_reprojection_loss_fwd(const double* M, const double* intr, const void* xy, int xy_dtype,
                                          int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                                          const double* omega, int G, int V, int J, int undistort, double* loss,
                                          double* X, double* e, void* workspace, long long workspace_bytes,
                                          void* stream) {
  POSU_REQUIRE(M && intr && xy && loss && workspace, "posu_reprojection_loss_fwd: null pointer");
  POSU_REQUIRE_TRI("posu_reprojection_loss_fwd");
  POSU_REQUIRE(workspace_bytes >= posu_reprojection_loss_workspace(G, J),
               "posu_reprojection_loss_fwd: workspace too small");
  POSU_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % sizeof(double) == 0,
               "posu_reprojection_loss_fwd: workspace must be 8-byte aligned");
  if (G == 0) return POSU_OK;
  const int blocks = (G * J + kLossBlock - 1) / kLossBlock;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(reprojection_fwd_kernel, dim3(blocks), dim3(kLossBlock), 0, as_stream(stream), M, intr, xy,
                     xy_dtype, xy_stride_g, xy_stride_v, vis, w, omega, G, V, J, undistort, part, X, e);
  hipLaunchKernelGGL(reprojection_sum_kernel, dim3(1), dim3(kLossBlock), 0, as_stream(stream), part, blocks,
                     static_cast<double>(G) * V * J, loss);
  return check_launch("posu_reprojection_loss_fwd");
}

extern "C" int posu_reprojection_loss_bwd(const double* M, const double* intr, const void* xy, int xy_dtype,
                                          int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                                          const double* omega, int G, int V, int J, int undistort, int detach_point,
                                          const double* gloss, void* gxy, double* gw, void* stream) {
  POSU_REQUIRE(M && intr && xy && gloss && gxy, "posu_reprojection_loss_bwd: null pointer");
  POSU_REQUIRE_TRI("posu_reprojection_loss_bwd");
  if (G == 0) return POSU_OK;
  hipLaunchKernelGGL(reprojection_bwd_kernel, dim3((G * J + 63) / 64), dim3(64), 0, as_stream(stream), M, intr, xy,
                     xy_dtype, xy_stride_g, xy_stride_v, vis, w, omega, G, V, J, undistort, detach_point, gloss, gxy,
                     gw);
  return check_launch("posu_reprojection_loss_bwd");
}
