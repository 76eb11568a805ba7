// What the training loop (lib/core/function.py:91-527) computes about a step besides the losses, on
// the device, so that the loop reads nothing back between two log lines:
//
//   posu_pck_accuracy   : PCK accuracy of V views' heatmaps against their targets
//                         (core/evaluate.py:17-73 over core/inference.py:19-47)
//   posu_grad_row_norms : the gradient-norm watch (utils/gradients.py:31-39)
//   posu_meters_update  : AverageMeter.update for every meter of the loop (function.py:705-709)
//
// No allocation, no synchronisation, no atomics; f64 partials summed in a fixed order (two calls on
// the same inputs give the same bits); one wave64 per map / four per gradient row.
#include "argmax_map.h"
#include "pck_common.h"
#include "posu_common.h"

namespace posu {
namespace {

constexpr int kMaxMeters = 64;   // kMaxViews: pck_common.h

struct ViewMaps {
  const float* out[kMaxViews];
  const float* tgt[kMaxViews];
};
struct ViewGrads {
  const float* g[kMaxViews];
};

// ---------------------------------------------------------------- PCK accuracy
// one wave per (view, n, j): both argmaxes, the prediction, and the pair's (valid, hit) flags
__global__ __launch_bounds__(64) void pck_pairs_kernel(ViewMaps views, int NJ, int H, int W, double thr,
                                                       float* __restrict__ pred, int* __restrict__ flags) {
  const int v = blockIdx.x / NJ, map = blockIdx.x - v * NJ;
  const int lane = threadIdx.x;
  const int HW = H * W;
  float ob, tb;
  int oi, ti;
  wave_argmax<true>(views.out[v] + static_cast<size_t>(map) * HW, HW, lane, ob, oi);
  wave_argmax<true>(views.tgt[v] + static_cast<size_t>(map) * HW, HW, lane, tb, ti);
  if (lane != 0) return;
  float pxf, pyf, txf, tyf;
  argmax_coords(ob, oi, W, pxf, pyf);
  argmax_coords(tb, ti, W, txf, tyf);
  pred[2 * static_cast<size_t>(blockIdx.x)] = pxf;
  pred[2 * static_cast<size_t>(blockIdx.x) + 1] = pyf;
  flags[blockIdx.x] = pck_pair_flags(pxf, pyf, txf, tyf, H, W, thr);   // pck_common.h
}

// ---------------------------------------------------------------- gradient row norms
// one 256-thread block per (view, row): sum |g| (p = 1) or g^2 (p = 2) in f64, thread t over the
// elements t, t + 256, .. (groups of four with 16-B loads), lanes then waves in a fixed order
template <int P>
__global__ __launch_bounds__(256) void row_norm_kernel(ViewGrads grads, int N, long long L,
                                                       double* __restrict__ rownorm) {
  const int v = blockIdx.x / N, n = blockIdx.x - v * N;
  const float* g = grads.g[v];
  if (!g) return;  // a view without a gradient
  g += static_cast<size_t>(n) * L;
  auto term = [](float x) {
    const double d = x;
    return P == 1 ? fabs(d) : d * d;
  };
  double s = 0.0;
  if ((L & 3) == 0 && (reinterpret_cast<size_t>(g) & 15) == 0) {
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (long long i = threadIdx.x; i < L / 4; i += 256) {
      const float4 x = g4[i];
      s += (term(x.x) + term(x.y)) + (term(x.z) + term(x.w));
    }
  } else {
    for (long long i = threadIdx.x; i < L; i += 256) s += term(g[i]);
  }
  __shared__ double part[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = (part[0] + part[1]) + (part[2] + part[3]);
    rownorm[blockIdx.x] = P == 1 ? t : __dsqrt_rn(t);
  }
}

// out = sum over the views that have a gradient of (sum of row norms / rows with a norm != 0),
// rows and views in index order (gradients.py:31-39); 0 / 0 = NaN for an all-zero view
__global__ __launch_bounds__(64) void row_norm_final_kernel(ViewGrads grads, int V, int N,
                                                            const double* __restrict__ rownorm,
                                                            double* __restrict__ out) {
  __shared__ double res[kMaxViews];
  const int v = threadIdx.x;
  if (v < V && grads.g[v]) {
    double s = 0.0, c = 0.0;
    for (int n = 0; n < N; ++n) {
      const double r = rownorm[static_cast<size_t>(v) * N + n];
      s = __dadd_rn(s, r);
      c += (r != 0.0) ? 1.0 : 0.0;
    }
    res[v] = s / c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < V; ++i)
      if (grads.g[i]) t = __dadd_rn(t, res[i]);
    out[0] = t;
  }
}

// ---------------------------------------------------------------- meters
// AverageMeter.update (function.py:705-709) of every active slot: val = v, sum += v * w, count += w
// (avg = sum / count is the reader's one division); product and sums rounded one by one, like the
// host's Python floats
__global__ __launch_bounds__(64) void meters_kernel(double* __restrict__ table, int M,
                                                    const double* __restrict__ val, const double* __restrict__ w,
                                                    unsigned long long active) {
  const int m = threadIdx.x;
  if (m >= M || !((active >> m) & 1ull)) return;
  double* t = table + 3 * m;
  const double x = val[m], n = w[m];
  t[0] = x;
  t[1] = __dadd_rn(t[1], __dmul_rn(x, n));
  t[2] = __dadd_rn(t[2], n);
}

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" long long posu_pck_accuracy_workspace(int V, int N, int J) {
  if (V < 1 || V > kMaxViews || N < 1 || J < 1) return -1;
  const long long pairs = static_cast<long long>(V) * N * J;
  if (pairs >= (1LL << 31)) return -1;
  return pairs * static_cast<long long>(sizeof(int));
}

extern "C" int posu_pck_accuracy(const float* const* outputs, const float* const* targets, int V, int N, int J,
                                 int H, int W, double thr, double* acc, double* avg, int* cnt, float* pred,
                                 double* step, void* workspace, long long workspace_bytes, void* stream) {
  POSU_REQUIRE(outputs && targets && acc && avg && cnt && pred && step && workspace,
               "posu_pck_accuracy: null pointer");
  POSU_REQUIRE(V >= 1 && V <= kMaxViews, "posu_pck_accuracy: 1 to 8 views");
  POSU_REQUIRE(N > 0 && J > 0 && H > 0 && W > 0 && static_cast<long long>(H) * W < (1LL << 31),
               "posu_pck_accuracy: bad shape");
  const long long need = posu_pck_accuracy_workspace(V, N, J);
  POSU_REQUIRE(need > 0, "posu_pck_accuracy: shape too large");
  POSU_REQUIRE(workspace_bytes >= need, "posu_pck_accuracy: workspace too small");
  POSU_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "posu_pck_accuracy: workspace must be 4-byte aligned");
  POSU_REQUIRE(((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(avg) |
                 reinterpret_cast<uintptr_t>(step)) & 7) == 0,
               "posu_pck_accuracy: acc, avg and step must be 8-byte aligned");
  ViewMaps views = {};
  for (int v = 0; v < V; ++v) {
    POSU_REQUIRE(outputs[v] && targets[v], "posu_pck_accuracy: null view pointer");
    views.out[v] = outputs[v];
    views.tgt[v] = targets[v];
  }
  hipStream_t s = as_stream(stream);
  int* flags = static_cast<int*>(workspace);
  hipLaunchKernelGGL(pck_pairs_kernel, dim3(static_cast<unsigned>(V) * N * J), dim3(64), 0, s, views, N * J, H, W,
                     thr, pred, flags);
  hipLaunchKernelGGL(pck_view_kernel, dim3(V), dim3(64), 0, s, flags, N, J, acc, avg, cnt);
  hipLaunchKernelGGL(pck_step_kernel, dim3(1), dim3(64), 0, s, avg, cnt, V, step);
  return check_launch("posu_pck_accuracy");
}

extern "C" long long posu_grad_row_norms_workspace(int V, int N) {
  if (V < 1 || V > kMaxViews || N < 1) return -1;
  return static_cast<long long>(V) * N * static_cast<long long>(sizeof(double));
}

extern "C" int posu_grad_row_norms(const float* const* grads, int V, int N, long long L, int p, double* out,
                                   void* workspace, long long workspace_bytes, void* stream) {
  POSU_REQUIRE(grads && out && workspace, "posu_grad_row_norms: null pointer");
  POSU_REQUIRE(V >= 1 && V <= kMaxViews, "posu_grad_row_norms: 1 to 8 views");
  POSU_REQUIRE(N > 0 && L > 0 && static_cast<long long>(V) * N < (1LL << 31), "posu_grad_row_norms: bad shape");
  POSU_REQUIRE(p == 1 || p == 2, "posu_grad_row_norms: norm order 1 or 2");
  POSU_REQUIRE(workspace_bytes >= posu_grad_row_norms_workspace(V, N), "posu_grad_row_norms: workspace too small");
  POSU_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
               "posu_grad_row_norms: workspace and out must be 8-byte aligned");
  ViewGrads g = {};
  for (int v = 0; v < V; ++v) g.g[v] = grads[v];
  hipStream_t s = as_stream(stream);
  double* rownorm = static_cast<double*>(workspace);
  if (p == 1)
    hipLaunchKernelGGL(row_norm_kernel<1>, dim3(static_cast<unsigned>(V) * N), dim3(256), 0, s, g, N, L, rownorm);
  else
    hipLaunchKernelGGL(row_norm_kernel<2>, dim3(static_cast<unsigned>(V) * N), dim3(256), 0, s, g, N, L, rownorm);
  hipLaunchKernelGGL(row_norm_final_kernel, dim3(1), dim3(64), 0, s, g, V, N, rownorm, out);
  return check_launch("posu_grad_row_norms");
}

extern "C" int posu_meters_update(double* table, int M, const double* v, const double* w,
                                  const unsigned char* active, void* stream) {
  POSU_REQUIRE(table && v && w && active, "posu_meters_update: null pointer");
  POSU_REQUIRE(M >= 1 && M <= kMaxMeters, "posu_meters_update: 1 to 64 meters");
  POSU_REQUIRE(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(w)) &
                7) == 0,
               "posu_meters_update: table, v and w must be 8-byte aligned");
  unsigned long long mask = 0;
  for (int m = 0; m < M; ++m)
    if (active[m]) mask |= 1ull << m;
  hipLaunchKernelGGL(meters_kernel, dim3(1), dim3(64), 0, as_stream(stream), table, M, v, w, mask);
  return check_launch("posu_meters_update");
}
