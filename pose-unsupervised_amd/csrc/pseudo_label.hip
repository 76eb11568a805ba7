// The pseudo-label round of run/test/test_pseudo_label.py:193-259 for a whole sweep of confidence
// thresholds: one launch that thresholds, runs RANSAC over the view pairs and re-projects, and one
// launch that reduces every label set to the integer counts behind PCKh, coverage and Joints@k.
//
// What the sweep shares: for one (group, joint) a pair's triangulation, its reprojection errors in
// the V views, hence its inlier set and mean inlier error, depend on the cameras, the predictions and
// REPROJ_THRE -- not on the confidence threshold, which only decides which pairs are eligible.  The
// (up to six) pairs are therefore solved once per thread and kept as (inlier mask, count, mean error)
// in registers; each threshold then costs a handful of integer tests, and the n-view DLT of the
// reprojection stage is solved again only when its visibility mask changed.
//
// The arithmetic is shared by construction: score_pair, BestPair and solve_project (geometry_common.h)
// are the functions posu_ransac_inliers / posu_reproject inline, so the masks and projections of one
// threshold are those two entry points' results on that threshold's mask.
#include "geometry_common.h"

namespace posu {
namespace {

constexpr int kMaxThre = 8;
constexpr int kPairs = kPairViews * (kPairViews - 1) / 2;

struct Thresholds {
  float v[kMaxThre];
};

__global__ __launch_bounds__(64) void sweep_kernel(const double* __restrict__ Mall, const double* __restrict__ intr,
                                                   const double* __restrict__ xy, const float* __restrict__ conf,
                                                   const Thresholds thre, int T, int G, int V, int J, int undistort,
                                                   double reproj_thre, int min_inliers, int use_ransac,
                                                   unsigned char* __restrict__ vis_out, double* __restrict__ proj_out) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= G * J) return;
  const int g = t / J, k = t - g * J;
  // every view is loaded and undistorted: a view's undistorted point does not depend on which
  // other views are visible
  ViewPts p;
  load_views(Mall, intr, xy, nullptr, g, k, V, J, undistort, p);
  float c[kPairViews];
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) c[v] = v < V ? conf[(static_cast<size_t>(g) * V + v) * J + k] : 0.f;

  // the pairs, in itertools.combinations order; view indices are compile-time (loops unrolled) so
  // that p's arrays and the pair tables stay in registers, as in ransac_kernel
  int pair_mask[kPairs], pair_n[kPairs];
  double pair_err[kPairs];
  {
    int q = 0;
#pragma unroll
    for (int a = 0; a < kPairViews; ++a) {
#pragma unroll
      for (int b = a + 1; b < kPairViews; ++b, ++q) {
        pair_mask[q] = 0;
        pair_n[q] = 0;
        pair_err[q] = 0.0;
        if (b >= V) continue;
        const PairScore s = score_pair(Mall, intr, p, g, V, a, b, reproj_thre);
        pair_mask[q] = s.mask;
        pair_n[q] = s.n;
        if (s.n > 0) pair_err[q] = s.err_sum / s.n;
      }
    }
  }

  const size_t GVJ = static_cast<size_t>(G) * V * J;
  const int all = (1 << V) - 1;
  int solved = -1;  // the mask whose n-view solve pj holds
  double pj[kPairViews][2];
#pragma unroll
  for (int v = 0; v < kPairViews; ++v) pj[v][0] = pj[v][1] = 0.0;

  for (int ti = 0; ti < T; ++ti) {
    // stage 0: numpy compares an f32 array with a Python float in f32
    const float th = thre.v[ti];
    int m0 = 0;
#pragma unroll
    for (int v = 0; v < kPairViews; ++v)
      if (v < V && c[v] > th) m0 |= 1 << v;

    // stage 1 (triangulate.py:102-165): pairs of visible views; more inliers wins, then the
    // smaller mean error; fewer than two visible views leave zeros
    BestPair best;
    {
      int q = 0;
#pragma unroll
      for (int a = 0; a < kPairViews; ++a) {
#pragma unroll
        for (int b = a + 1; b < kPairViews; ++b, ++q) {
          if (!((m0 >> a) & 1) || !((m0 >> b) & 1)) continue;
          if (pair_n[q] < min_inliers) continue;
          best.offer(pair_mask[q], pair_n[q], pair_err[q]);
        }
      }
    }
    const int m1 = best.mask;

    // stage 2 (triangulate.py:169-213) on the stage-1 mask with RANSAC, else on the stage-0 mask
    const int src = use_ransac ? m1 : m0;
    const bool ok = __popc(src) >= 2;
    if (ok && src != solved) {
      solve_project(Mall, intr, p, g, V, src, pj);
      solved = src;
    }
    const int m2 = ok ? all : 0;

    unsigned char* vo = vis_out + static_cast<size_t>(ti) * 3 * GVJ;
    double* po = proj_out + static_cast<size_t>(ti) * GVJ * 2;
#pragma unroll
    for (int v = 0; v < kPairViews; ++v) {
      if (v >= V) break;
      const size_t e = (static_cast<size_t>(g) * V + v) * J + k;
      vo[e] = (m0 >> v) & 1;
      vo[GVJ + e] = (m1 >> v) & 1;
      vo[2 * GVJ + e] = (m2 >> v) & 1;
      po[2 * e] = ok ? pj[v][0] : 0.0;
      po[2 * e + 1] = ok ? pj[v][1] : 0.0;
    }
  }
}

// ------------------------------------------------------------------ counts
constexpr int kMaxSets = 32;
constexpr int kMaxCountViews = 8;

struct SetPred {
  int v[kMaxSets];
};

// One wave per (64 groups, label set): lane = group, joints in a loop.  Per joint the lanes' counts
// are added across the wave and lane 0 issues one atomicAdd per non-zero counter; the histogram of
// visible views per (group, joint) is kept per lane over the joints and reduced once at the end.
__global__ __launch_bounds__(64) void pckh_counts_kernel(const double* __restrict__ pred,
                                                         const double* __restrict__ pred_sets, const SetPred sel,
                                                         const unsigned char* __restrict__ vis,
                                                         const double* __restrict__ gt,
                                                         const double* __restrict__ head, int G, int V, int J,
                                                         double threshold, int* __restrict__ counts) {
  const int b = blockIdx.y;
  const int g = blockIdx.x * 64 + threadIdx.x;
  const bool live = g < G;
  const size_t NJ = static_cast<size_t>(G) * V * J;
  const int s = sel.v[b];
  const double* pr = s < 0 ? pred : pred_sets + static_cast<size_t>(s) * NJ * 2;
  const unsigned char* vs = vis + static_cast<size_t>(b) * NJ;
  int* out = counts + static_cast<size_t>(b) * (2 * J + V + 1);
  int hist[kMaxCountViews + 1];
#pragma unroll
  for (int i = 0; i <= kMaxCountViews; ++i) hist[i] = 0;
  for (int j = 0; j < J; ++j) {
    int nd = 0, nv = 0;
    if (live) {
      for (int v = 0; v < V; ++v) {
        const size_t f = static_cast<size_t>(g) * V + v;
        if (!vs[f * J + j]) continue;
        ++nv;
        if (!gt) continue;
        // np.sqrt(np.sum((gt - pred)**2, axis=2)) / headsize <= threshold, each operation rounded
        // on its own as numpy does (no contraction into an fma)
        const size_t e = (f * J + j) * 2;
        const double dx = gt[e] - pr[e], dy = gt[e + 1] - pr[e + 1];
        const double d = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
        if (d / head[f] <= threshold) ++nd;
      }
#pragma unroll
      for (int i = 0; i <= kMaxCountViews; ++i) hist[i] += nv == i;
    }
    nd = wave_sum(nd);
    nv = wave_sum(nv);
    if (threadIdx.x == 0) {
      if (nd) atomicAdd(out + j, nd);
      if (nv) atomicAdd(out + J + j, nv);
    }
  }
#pragma unroll
  for (int i = 0; i <= kMaxCountViews; ++i) {
    const int h = wave_sum(hist[i]);
    if (threadIdx.x == 0 && i <= V && h) atomicAdd(out + 2 * J + i, h);
  }
}

bool sweep_shape_ok(int T, int G, int V, int J) {
  return T >= 1 && T <= kMaxThre && V >= 2 && V <= kPairViews && J > 0 && G >= 0;
}

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" long long posu_pseudo_label_workspace(int T, int G, int V, int J) {
  if (!sweep_shape_ok(T, G, V, J)) return -1;
  const long long gvj = static_cast<long long>(G) * V * J;
  const long long proj = static_cast<long long>(T) * gvj * 2 * 8;
  const long long counts = static_cast<long long>(T) * 3 * (2 * J + V + 1) * 4;
  const long long masks = static_cast<long long>(T) * 3 * gvj;
  return proj + (counts + 7) / 8 * 8 + masks;
}

extern "C" int posu_pseudo_label_sweep(const double* M, const double* intr, const double* xy, const float* conf,
                                       const float* thre, int T, int G, int V, int J, int undistort,
                                       double reproj_thre, int min_inliers, int use_ransac, unsigned char* vis_out,
                                       double* proj_out, void* stream) {
  POSU_REQUIRE(sweep_shape_ok(T, G, V, J), "posu_pseudo_label_sweep: bad shape (1 <= T <= 8, 2 <= V <= 4, J > 0)");
  POSU_REQUIRE(min_inliers >= 1,
               "posu_pseudo_label_sweep: min_inliers >= 1 (the reference divides by the inlier count)");
  POSU_REQUIRE(static_cast<long long>(G) * J <= 0x7fffffffLL - 64, "posu_pseudo_label_sweep: G * J too large");
  if (G == 0) return POSU_OK;  // nothing to read or write: empty tensors have no address
  POSU_REQUIRE(M && intr && xy && conf && thre && vis_out && proj_out, "posu_pseudo_label_sweep: null pointer");
  Thresholds th;
  for (int i = 0; i < kMaxThre; ++i) th.v[i] = i < T ? thre[i] : 0.f;
  hipLaunchKernelGGL(sweep_kernel, dim3((G * J + 63) / 64), dim3(64), 0, as_stream(stream), M, intr, xy, conf, th, T,
                     G, V, J, undistort, reproj_thre, min_inliers, use_ransac, vis_out, proj_out);
  return check_launch("posu_pseudo_label_sweep");
}

extern "C" int posu_pckh_counts(const double* pred, const double* pred_sets, const int* set_pred,
                                const unsigned char* vis, const double* gt, const double* head, int B, int N, int J,
                                int V, double threshold, int* counts, void* stream) {
  POSU_REQUIRE(counts, "posu_pckh_counts: null pointer");
  POSU_REQUIRE(B >= 1 && B <= kMaxSets && N >= 0 && J > 0 && V >= 1 && V <= kMaxCountViews && N % V == 0,
               "posu_pckh_counts: bad shape (1 <= B <= 32, 1 <= V <= 8, N a multiple of V, J > 0)");
  POSU_REQUIRE(static_cast<long long>(N) * J <= 0x7fffffffLL, "posu_pckh_counts: N * J too large");
  POSU_REQUIRE(N == 0 || vis, "posu_pckh_counts: null pointer");
  POSU_REQUIRE(N == 0 || !gt || head, "posu_pckh_counts: null pointer (head goes with gt)");
  SetPred sel;
  for (int i = 0; i < kMaxSets; ++i) {
    sel.v[i] = (set_pred && i < B) ? set_pred[i] : -1;
    POSU_REQUIRE(N == 0 || !gt || (sel.v[i] < 0 ? (i >= B || pred != nullptr) : pred_sets != nullptr),
                 "posu_pckh_counts: null pointer (a set's predictions)");
  }
  const size_t bytes = static_cast<size_t>(B) * (2 * J + V + 1) * sizeof(int);
  const hipError_t e = hipMemsetAsync(counts, 0, bytes, as_stream(stream));
  if (e != hipSuccess) {
    set_error(std::string("posu_pckh_counts: ") + hipGetErrorString(e));
    return POSU_ERR_HIP;
  }
  if (N == 0) return POSU_OK;
  const int G = N / V;
  hipLaunchKernelGGL(pckh_counts_kernel, dim3((G + 63) / 64, B), dim3(64), 0, as_stream(stream), pred, pred_sets,
                     sel, vis, gt, head, G, V, J, threshold, counts);
  return check_launch("posu_pckh_counts");
}
