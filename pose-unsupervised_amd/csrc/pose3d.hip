// The 3-D evaluation protocol of run/pose3d/estimate.py as fp64 kernels: Procrustes alignment
// (PoseUtils.procrustes, lib/utils/pose_utils.py:61-143), the per-camera joint errors
// (error_computing_3d, estimate.py:110-123) and the limb-length check (break_limb_length,
// estimate.py:84-96).  Latency-bound, tiny working sets: one wave per pose, lanes stride over the
// joints (so J may exceed 64), every sum a wave reduction (posu_common.h); no LDS, no atomics.
//
// Procrustes follows the reference's order of operations: subtract the means, ssX / ssY and the
// norms, divide by them, M = A0^T B0, SVD, R = V U^T, S_trace = sum s, then scale / d / Z /
// translation (the second branch with scaling off).  The 3 x 3 SVD is jacobi_columns
// (geometry_common.h), the loop dlt_point runs: on return the column norms of M are the singular
// values and the normalised columns are U.  Every matrix is indexed by compile-time constants only
// (a run-time index would put it in scratch).  At most 30 sweeps, and the rotation test is false
// for NaN, so a degenerate pose (all joints equal: 0 / 0) ends with NaN rows instead of spinning.
// For a rank-2 M (coplanar joints) the missing column of U is the cross product of the other two,
// where LAPACK completes the basis with a sign of its choice; collinear joints (rank 1) have no
// defined result.
#include "geometry_common.h"

namespace posu {
namespace {

constexpr int kWavesPerBlock = 4;

// the rigid (or similarity) transform of one pose pair, identical in every lane of the wave
struct Tform {
  double a_bar[3], b_bar[3];
  double b_norm;   // sqrt(ssY): B0 = (B - b_bar) / b_norm
  double z_scale;  // Z = z_scale * (B0 R) + a_bar
  double R[3][3];
  double scale, d;
};

// M = U diag(s) V^T by jacobi_columns on M's columns -> R = V U^T and s sorted descending
// (numpy's order: s[2] is the one the forced reflection negates).  flip: 0 keep, 1 force a
// reflection, 2 forbid one (pose_utils.py:111-119).
__device__ __forceinline__ void rotation_from(double (&W)[3][3], int flip, double (&R)[3][3], double (&s)[3]) {
  double V[3][3];
  jacobi_columns<3, 3>(W, V);
  double sv[3], U[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sv[c] = sqrt(W[0][c] * W[0][c] + W[1][c] * W[1][c] + W[2][c] * W[2][c]);
#pragma unroll
    for (int r = 0; r < 3; ++r) U[r][c] = W[r][c] / sv[c];
  }
  // the column of the smallest singular value (the last such column on a tie)
  int kmin = 0;
  double smin = sv[0];
#pragma unroll
  for (int c = 1; c < 3; ++c) {
    if (sv[c] <= smin) {
      smin = sv[c];
      kmin = c;
    }
  }
  const double smax = fmax(sv[0], fmax(sv[1], sv[2]));
  // rank 2 (coplanar joints: the column is zero or rounding noise, its quotient above 0 / 0 or no
  // direction): that column of U is the cross product of the other two, where LAPACK completes the
  // basis with a sign of its choice.  Not taken by a well-conditioned M; NaN stays NaN.
  if (!(smin > 1e-14 * smax)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c == kmin) {
        const int a = (c + 1) % 3, b = (c + 2) % 3;
        U[0][c] = U[1][a] * U[2][b] - U[2][a] * U[1][b];
        U[1][c] = U[2][a] * U[0][b] - U[0][a] * U[2][b];
        U[2][c] = U[0][a] * U[1][b] - U[1][a] * U[0][b];
      }
    }
  }
  double sign[3] = {1.0, 1.0, 1.0};
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        R[i][j] = sign[0] * V[i][0] * U[j][0] + sign[1] * V[i][1] * U[j][1] + sign[2] * V[i][2] * U[j][2];
    }
    if (pass == 1 || flip == 0) break;
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) -
                       R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    const bool have = det < 0.0;
    if ((flip == 1) == have) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) sign[c] = c == kmin ? -1.0 : 1.0;
  }
  s[0] = smax;
  s[2] = smin * (sign[0] * sign[1] * sign[2]);
  // the middle one: what is left of the three (exact when two coincide with max / min bit for bit)
  s[1] = kmin == 0 ? fmin(sv[1], sv[2]) : (kmin == 1 ? fmin(sv[0], sv[2]) : fmin(sv[0], sv[1]));
}

// PoseUtils.procrustes(A, B) for the pose of this wave.  loadA(j, a) / loadB(j, b) fetch joint j.
template <typename LA, typename LB>
__device__ __forceinline__ void procrustes_wave(LA loadA, LB loadB, int J, int lane, int scaling, int flip,
                                                Tform& f) {
  double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
  for (int j = lane; j < J; j += 64) {
    double a[3], b[3];
    loadA(j, a);
    loadB(j, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sa[c] += a[c];
      sb[c] += b[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f.a_bar[c] = wave_sum(sa[c]) / J;
    f.b_bar[c] = wave_sum(sb[c]) / J;
  }
  double ssx = 0, ssy = 0;
  for (int j = lane; j < J; j += 64) {
    double a[3], b[3];
    loadA(j, a);
    loadB(j, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a0 = a[c] - f.a_bar[c], b0 = b[c] - f.b_bar[c];
      ssx += a0 * a0;
      ssy += b0 * b0;
    }
  }
  ssx = wave_sum(ssx);
  ssy = wave_sum(ssy);
  const double a_norm = sqrt(ssx);
  f.b_norm = sqrt(ssy);
  double m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int j = lane; j < J; j += 64) {
    double a[3], b[3];
    loadA(j, a);
    loadB(j, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a[c] = (a[c] - f.a_bar[c]) / a_norm;
      b[c] = (b[c] - f.b_bar[c]) / f.b_norm;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) m[r][c] += a[r] * b[c];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) m[r][c] = wave_sum(m[r][c]);
  double s[3];
  rotation_from(m, flip, f.R, s);
  const double s_trace = (s[0] + s[1]) + s[2];
  if (scaling) {
    f.scale = s_trace * a_norm / f.b_norm;
    f.d = 1.0 - s_trace * s_trace;
    f.z_scale = a_norm * s_trace;
  } else {
    f.scale = 1.0;
    f.d = 1.0 + ssy / ssx - 2.0 * s_trace * f.b_norm / a_norm;
    f.z_scale = f.b_norm;
  }
}

// row j of Z = z_scale * (B0 R) + a_bar
__device__ __forceinline__ void align_joint(const Tform& f, const double* b, double* z) {
  double b0[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) b0[c] = (b[c] - f.b_bar[c]) / f.b_norm;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    z[c] = f.z_scale * (b0[0] * f.R[0][c] + b0[1] * f.R[1][c] + b0[2] * f.R[2][c]) + f.a_bar[c];
}

__device__ __forceinline__ void load3(const double* p, double* v) {
  v[0] = p[0];
  v[1] = p[1];
  v[2] = p[2];
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void procrustes_kernel(
    const double* __restrict__ A, const double* __restrict__ B, int N, int J, int scaling, int flip,
    double* __restrict__ d, double* __restrict__ Z, double* __restrict__ R, double* __restrict__ scale,
    double* __restrict__ t) {
  const int n = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;  // wave-uniform
  const double* a = A + static_cast<size_t>(n) * J * 3;
  const double* b = B + static_cast<size_t>(n) * J * 3;
  auto la = [a](int j, double* v) { load3(a + 3 * j, v); };
  auto lb = [b](int j, double* v) { load3(b + 3 * j, v); };
  Tform f;
  procrustes_wave(la, lb, J, lane, scaling, flip, f);
  if (Z) {
    double* z = Z + static_cast<size_t>(n) * J * 3;
    for (int j = lane; j < J; j += 64) {
      double bj[3], zj[3];
      lb(j, bj);
      align_joint(f, bj, zj);
      z[3 * j] = zj[0];
      z[3 * j + 1] = zj[1];
      z[3 * j + 2] = zj[2];
    }
  }
  if (lane == 0) {
    if (d) d[n] = f.d;
    if (scale) scale[n] = f.scale;
    if (R) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[static_cast<size_t>(n) * 9 + 3 * i + j] = f.R[i][j];
    }
    if (t) {  // translation = A_bar - scale * (B_bar R)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        t[static_cast<size_t>(n) * 3 + c] =
            f.a_bar[c] - f.scale * (f.b_bar[0] * f.R[0][c] + f.b_bar[1] * f.R[1][c] + f.b_bar[2] * f.R[2][c]);
    }
  }
}

// one wave per (group, camera): pred = (R (X^T - T))^T, optionally Procrustes-aligned onto gt
__global__ __launch_bounds__(64 * kWavesPerBlock) void pose3d_errors_kernel(
    const double* __restrict__ X, const double* __restrict__ gt, const double* __restrict__ Rc,
    const double* __restrict__ Tc, int GV, int V, int J, int procrustes, double* __restrict__ err,
    double* __restrict__ aligned) {
  const int gv = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (gv >= GV) return;  // wave-uniform
  const double* x = X + static_cast<size_t>(gv / V) * J * 3;
  const double* a = gt + static_cast<size_t>(gv) * J * 3;
  double Rm[9], Tv[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rm[i] = Rc[static_cast<size_t>(gv) * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) Tv[i] = Tc[static_cast<size_t>(gv) * 3 + i];
  auto la = [a](int j, double* v) { load3(a + 3 * j, v); };
  auto lb = [&](int j, double* v) {
    const double x0 = x[3 * j] - Tv[0], x1 = x[3 * j + 1] - Tv[1], x2 = x[3 * j + 2] - Tv[2];
    v[0] = Rm[0] * x0 + Rm[1] * x1 + Rm[2] * x2;
    v[1] = Rm[3] * x0 + Rm[4] * x1 + Rm[5] * x2;
    v[2] = Rm[6] * x0 + Rm[7] * x1 + Rm[8] * x2;
  };
  Tform f;
  if (procrustes) procrustes_wave(la, lb, J, lane, 1, 0, f);
  for (int j = lane; j < J; j += 64) {
    double g[3], p[3];
    la(j, g);
    lb(j, p);
    if (procrustes) {
      double z[3];
      align_joint(f, p, z);
      p[0] = z[0];
      p[1] = z[1];
      p[2] = z[2];
    }
    const double d0 = g[0] - p[0], d1 = g[1] - p[1], d2 = g[2] - p[2];
    const size_t o = static_cast<size_t>(gv) * J + j;
    err[o] = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    if (aligned) {
      aligned[3 * o] = p[0];
      aligned[3 * o + 1] = p[1];
      aligned[3 * o + 2] = p[2];
    }
  }
}

// one wave per group: lanes stride over the child joints
__global__ __launch_bounds__(64 * kWavesPerBlock) void limb_break_kernel(
    const double* __restrict__ X, const int* __restrict__ parent, const double* __restrict__ limb, int limb_stride,
    int G, int J, double thres, unsigned char* __restrict__ flag, double* __restrict__ worst) {
  const int g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= G) return;  // wave-uniform
  const double* x = X + static_cast<size_t>(g) * J * 3;
  const double* L = limb + static_cast<size_t>(g) * limb_stride;
  int broke = 0;
  double w = 0.0;
  for (int c = lane; c < J; c += 64) {
    const int p = parent[c];
    if (p < 0 || p >= J) continue;  // the root (or no joint of this pose): no limb
    const double d0 = x[3 * p] - x[3 * c], d1 = x[3 * p + 1] - x[3 * c + 1], d2 = x[3 * p + 2] - x[3 * c + 2];
    const double expect = L[c];
    const double offset = fabs(expect - sqrt(d0 * d0 + d1 * d1 + d2 * d2));
    if (offset > thres * expect) broke = 1;  // strict; false for NaN, as in numpy
    const double rel = offset / expect;
    if (rel > w) w = rel;
  }
  w = wave_max(w);  // never NaN: the comparison above is false for one
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) broke |= __shfl_xor(broke, o, 64);
  if (lane == 0) {
    flag[g] = static_cast<unsigned char>(broke);
    if (worst) worst[g] = w;
  }
}

inline int wave_blocks(int waves) { return (waves + kWavesPerBlock - 1) / kWavesPerBlock; }

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" int posu_procrustes(const double* A, const double* B, int N, int J, int scaling, int reflection, double* d,
                               double* Z, double* R, double* scale, double* t, void* stream) {
  POSU_REQUIRE(A && B, "posu_procrustes: null pointer");
  POSU_REQUIRE(d || Z || R || scale || t, "posu_procrustes: null pointer (every output is null)");
  POSU_REQUIRE(N > 0 && J >= 1, "posu_procrustes: bad shape (N > 0, J >= 1)");
  POSU_REQUIRE(reflection >= 0 && reflection <= 2, "posu_procrustes: reflection must be 0 (best), 1 (force) or 2 (forbid)");
  hipLaunchKernelGGL(procrustes_kernel, dim3(wave_blocks(N)), dim3(64 * kWavesPerBlock), 0, as_stream(stream), A, B, N,
                     J, scaling != 0, reflection, d, Z, R, scale, t);
  return check_launch("posu_procrustes");
}

extern "C" int posu_pose3d_errors(const double* X, const double* gt, const double* R, const double* T, int G, int V,
                                  int J, int procrustes, double* err, double* aligned, void* stream) {
  POSU_REQUIRE(X && gt && R && T && err, "posu_pose3d_errors: null pointer");
  POSU_REQUIRE(G > 0 && V > 0 && J >= 1, "posu_pose3d_errors: bad shape (G > 0, V > 0, J >= 1)");
  POSU_REQUIRE(static_cast<long long>(G) * V <= 0x7fffffffLL, "posu_pose3d_errors: G * V too large");
  const int gv = G * V;
  hipLaunchKernelGGL(pose3d_errors_kernel, dim3(wave_blocks(gv)), dim3(64 * kWavesPerBlock), 0, as_stream(stream), X,
                     gt, R, T, gv, V, J, procrustes != 0, err, aligned);
  return check_launch("posu_pose3d_errors");
}

extern "C" int posu_limb_break(const double* X, const int* parent, const double* limb, int limb_stride, int G, int J,
                               double thres, unsigned char* flag, double* worst, void* stream) {
  POSU_REQUIRE(X && parent && limb && flag, "posu_limb_break: null pointer");
  POSU_REQUIRE(G > 0 && J >= 1, "posu_limb_break: bad shape (G > 0, J >= 1)");
  POSU_REQUIRE(limb_stride == 0 || limb_stride == J, "posu_limb_break: limb_stride must be 0 (shared) or J");
  hipLaunchKernelGGL(limb_break_kernel, dim3(wave_blocks(G)), dim3(64 * kWavesPerBlock), 0, as_stream(stream), X,
                     parent, limb, limb_stride, G, J, thres, flag, worst);
  return check_launch("posu_limb_break");
}
