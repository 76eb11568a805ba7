// PCK accuracy from per-pair flags (accuracy, lib/core/evaluate.py:42-73), shared by
// posu_pck_accuracy (train_metrics.hip) and posu_decode_views (validate.hip): the pair's flags from the
// two argmaxes, the per-view table and the step means.  The kernels live in an unnamed namespace:
// every translation unit that includes this header gets its own copy.
#pragma once
#include "posu_common.h"

namespace posu {
namespace {

constexpr int kMaxViews = 8;

// (valid, hit) of one (output, target) argmax pair as bit 0 / bit 1.  evaluate.py:17-29 in f64; x
// over H / 10 and y over W / 10 is the reference's pairing (evaluate.py:56 with :24-26).  Explicitly
// rounded products and sum: no contraction.
__device__ __forceinline__ int pck_pair_flags(float pxf, float pyf, float txf, float tyf, int H, int W, double thr) {
  const double px = pxf, py = pyf, tx = txf, ty = tyf;
  const double nx = static_cast<double>(H) / 10.0, ny = static_cast<double>(W) / 10.0;
  const bool valid = tx > 1.0 && ty > 1.0;
  const double dx = px / nx - tx / nx, dy = py / ny - ty / ny;
  const double d = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
  return (valid ? 1 : 0) | ((valid && d < thr) ? 2 : 0);
}

// one block per view: per joint the counts over n in index order and hits / valid; then the
// average joint by joint in index order over the joints that have a valid target
// (evaluate.py:59-72)
__global__ __launch_bounds__(64) void pck_view_kernel(const int* __restrict__ flags, int N, int J,
                                                      double* __restrict__ acc, double* __restrict__ avg,
                                                      int* __restrict__ cnt) {
  const int v = blockIdx.x;
  const int* f = flags + static_cast<size_t>(v) * N * J;
  double* a = acc + static_cast<size_t>(v) * (J + 1);
  for (int j = threadIdx.x; j < J; j += 64) {
    int nvalid = 0, nhit = 0;
    for (int n = 0; n < N; ++n) {
      const int b = f[static_cast<size_t>(n) * J + j];
      nvalid += b & 1;
      nhit += b >> 1;
    }
    a[j + 1] = nvalid ? static_cast<double>(nhit) / static_cast<double>(nvalid) : -1.0;
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int c = 0;
    for (int j = 0; j < J; ++j) {
      const double x = a[j + 1];
      if (x >= 0.0) {
        s = __dadd_rn(s, x);
        ++c;
      }
    }
    if (c) s = s / static_cast<double>(c);
    a[0] = c ? s : 0.0;
    avg[v] = s;
    cnt[v] = c;
  }
}

// np.mean over the views (function.py:467-468): numpy adds fewer than eight values one after the
// other and exactly eight as a tree of pairs
__device__ __forceinline__ double mean_like_numpy(const double* x, int n) {
  double s;
  if (n == 8) {
    s = __dadd_rn(__dadd_rn(__dadd_rn(x[0], x[1]), __dadd_rn(x[2], x[3])),
                  __dadd_rn(__dadd_rn(x[4], x[5]), __dadd_rn(x[6], x[7])));
  } else {
    s = 0.0;
    for (int i = 0; i < n; ++i) s = __dadd_rn(s, x[i]);
  }
  return s / static_cast<double>(n);
}

__global__ __launch_bounds__(64) void pck_step_kernel(const double* __restrict__ avg, const int* __restrict__ cnt,
                                                      int V, double* __restrict__ step) {
  if (threadIdx.x != 0) return;
  double a[kMaxViews], c[kMaxViews];
  for (int v = 0; v < V; ++v) {
    a[v] = avg[v];
    c[v] = static_cast<double>(cnt[v]);
  }
  step[0] = mean_like_numpy(a, V);
  step[1] = mean_like_numpy(c, V);
}

}  // namespace
}  // namespace posu
