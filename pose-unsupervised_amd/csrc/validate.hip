// The validation loop's batch body after the forwards (lib/core/function.py:567-644) and the counts behind
// the two dataset evaluations it ends with, on the device:
//
//   posu_decode_views     : for all V views of a batch in one launch the flip-test merge
//                           (flip_back_th transforms.py:33-47, SHIFT_HEATMAP function.py:579-583),
//                           get_final_preds (core/inference.py:19-75) and accuracy (core/evaluate.py:42-73),
//                           written straight into the epoch's preds / heatmaps buffers in the
//                           reference's preds[k::nviews] row order (function.py:632-644)
//   posu_detection_counts : per threshold and joint the rows within head-size distance of the ground truth
//                           (multiview_h36m_compatible.py:205-208, mpii_compatible.py:173-175)
//
// posu_decode_views uses the expressions of flip_back_kernel, argmax_kernel (heatmap.hip) and
// pck_pairs_kernel (train_metrics.hip): the same bits as that chain.  No allocation, no synchronisation;
// one wave64 per map.
#include "argmax_map.h"
#include "pck_common.h"
#include "posu_common.h"

namespace posu {
namespace {

struct DecodeViews {
  const float* out[kMaxViews];
  const float* flip[kMaxViews];  // all null: no flip test
  const float* tgt[kMaxViews];   // all null: no accuracy
};

// One merged map: m[i] = 0.5f * (o[i] + F), F = f[y][W - 1 - xs], xs = shift ? max(x - 1, 0) : x
// (flip_back_kernel's expression; f already points at joint perm[j]); m = o without a flipped map.
struct MergedMap {
  const float* o;
  const float* f;
  int W, shift;
  __device__ __forceinline__ float merge(float a, int y, int x) const {
    const int xs = shift ? (x > 0 ? x - 1 : 0) : x;
    return 0.5f * (a + f[y * W + (W - 1 - xs)]);
  }
  __device__ __forceinline__ float at(int i) const {
    if (!f) return o[i];
    const int y = i / W;
    return merge(o[i], y, i - y * W);
  }
};

// one wave per (view, n, j); blockIdx.x = (v * N + n) * J + j
__global__ __launch_bounds__(64) void decode_views_kernel(DecodeViews views, const int* __restrict__ perm, int V,
                                                          int N, int J, int H, int W, int shift, int post,
                                                          const double* __restrict__ aff, double thr,
                                                          long long row0, float* __restrict__ merged,
                                                          float* __restrict__ preds, int* __restrict__ flags) {
  const int NJ = N * J;
  const int v = blockIdx.x / NJ, map = blockIdx.x - v * NJ;
  const int n = map / J, j = map - n * J;
  const int lane = threadIdx.x;
  const int HW = H * W;
  MergedMap m;
  m.W = W;
  m.shift = shift;
  m.o = views.out[v] + static_cast<size_t>(map) * HW;
  m.f = nullptr;
  if (views.flip[v]) {
    int js = perm ? perm[j] : j;
    if (js < 0 || js >= J) js = j;  // a pair table that names no joint: the joint itself, never out of the map
    m.f = views.flip[v] + (static_cast<size_t>(n) * J + js) * HW;
  }
  const size_t row = static_cast<size_t>(row0) + static_cast<size_t>(n) * V + v;  // preds[k::nviews]
  float* mo = merged ? merged + (row * J + j) * HW : nullptr;

  float best = -INFINITY;
  int bidx = 0x7fffffff;
  auto take = [&](float a, int i) {
    if (a > best) {  // strict: the first (smallest) index of a tie within the lane
      best = a;
      bidx = i;
    }
  };
  // 16-B loads of o (and stores of the merged map) when a row is whole float4s and both maps are 16-B
  // aligned; the mirrored (and shifted) read stays on 4-B loads.  Either loop meets a lane's elements
  // in rising index order and merges with the same expression: the same map and (best, bidx).
  const bool vec4 = (HW & 3) == 0 && (W & 3) == 0 && (reinterpret_cast<size_t>(m.o) & 15) == 0 &&
                    (!mo || (reinterpret_cast<size_t>(mo) & 15) == 0);
  if (vec4) {
    const float4* o4 = reinterpret_cast<const float4*>(m.o);
    for (int i = lane; i < HW / 4; i += 64) {
      float4 a = o4[i];
      if (m.f) {
        const int y = (4 * i) / W, x = 4 * i - y * W;
        a.x = m.merge(a.x, y, x);
        a.y = m.merge(a.y, y, x + 1);
        a.z = m.merge(a.z, y, x + 2);
        a.w = m.merge(a.w, y, x + 3);
      }
      if (mo) reinterpret_cast<float4*>(mo)[i] = a;
      take(a.x, 4 * i);
      take(a.y, 4 * i + 1);
      take(a.z, 4 * i + 2);
      take(a.w, 4 * i + 3);
    }
  } else {
    for (int i = lane; i < HW; i += 64) {
      const float a = m.at(i);
      if (mo) mo[i] = a;
      take(a, i);
    }
  }
  wave_argmax_lanes(best, bidx);

  const float* t = views.tgt[v];  // the same for the whole wave
  float tb = 0.f;
  int ti = 0;
  if (t) wave_argmax<true>(t + static_cast<size_t>(map) * HW, HW, lane, tb, ti);
  if (lane != 0) return;

  float px, py;
  argmax_coords(best, bidx, W, px, py);
  if (t) {  // accuracy compares the plain argmaxes (evaluate.py:52-53)
    float tx, ty;
    argmax_coords(tb, ti, W, tx, ty);
    flags[blockIdx.x] = pck_pair_flags(px, py, tx, ty, H, W, thr);
  }
  if (post) {  // inference.py:56-67; the neighbours from the inputs: merged may be null
    const int ix = static_cast<int>(floorf(px + 0.5f)), iy = static_cast<int>(floorf(py + 0.5f));
    if (1 < ix && ix < W - 1 && 1 < iy && iy < H - 1) {
      const float dx = m.at(iy * W + ix + 1) - m.at(iy * W + ix - 1);
      const float dy = m.at((iy + 1) * W + ix) - m.at((iy - 1) * W + ix);
      px += (dx > 0.f ? 0.25f : (dx < 0.f ? -0.25f : 0.f));
      py += (dy > 0.f ? 0.25f : (dy < 0.f ? -0.25f : 0.f));
    }
  }
  float ox = px, oy = py;
  if (aff) {  // transform_preds with the f64 matrix, view-major [V * N, 2, 3]
    const double* T = aff + (static_cast<size_t>(v) * N + n) * 6;
    ox = static_cast<float>(static_cast<double>(px) * T[0] + static_cast<double>(py) * T[1] + T[2]);
    oy = static_cast<float>(static_cast<double>(px) * T[3] + static_cast<double>(py) * T[4] + T[5]);
  }
  float* p = preds + (row * J + j) * 3;
  p[0] = ox;
  p[1] = oy;
  p[2] = best;
}

// ------------------------------------------------------------------ detection counts
constexpr int kMaxDetThre = 8;

struct DetThresholds {
  double v[kMaxDetThre];
};

// One wave per 64 rows: lane = row, joints in a loop.  Per joint the lanes' flags are added across the
// wave and lane 0 issues one atomicAdd per non-zero counter (integers: the order does not matter).
__global__ __launch_bounds__(64) void detection_counts_kernel(const float* __restrict__ pred, int C,
                                                              const double* __restrict__ gt,
                                                              const double* __restrict__ head,
                                                              const unsigned char* __restrict__ vis,
                                                              DetThresholds thr, int T, int form, int N, int J,
                                                              int* __restrict__ counts) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  const bool live = n < N;
  const double h = live ? head[n] : 1.0;
  for (int j = 0; j < J; ++j) {
    const size_t e = static_cast<size_t>(live ? n : 0) * J + j;
    const bool seen = live && (!vis || vis[e]);
    double d = 0.0;
    if (seen) {
      // np.sqrt(np.sum((gt - pred)**2, axis=2)), each operation rounded on its own as numpy does
      const double dx = gt[2 * e] - static_cast<double>(pred[C * e]);
      const double dy = gt[2 * e + 1] - static_cast<double>(pred[C * e + 1]);
      d = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
    }
    const int nv = wave_sum(seen ? 1 : 0);
    for (int t = 0; t < T; ++t) {  // T is the same for every lane
      const double th = thr.v[t];
      const bool hit = seen && (form ? (d / h <= th) : (d <= __dmul_rn(h, th)));
      const int s = wave_sum(hit ? 1 : 0);
      if (threadIdx.x == 0) {
        int* out = counts + static_cast<size_t>(t) * 2 * J;
        if (s) atomicAdd(out + j, s);
        if (nv) atomicAdd(out + J + j, nv);
      }
    }
  }
}

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" long long posu_decode_views_workspace(int V, int N, int J) {
  if (V < 1 || V > kMaxViews || N < 0 || J < 1) return -1;
  const long long maps = static_cast<long long>(V) * N * J;
  if (maps >= (1LL << 31)) return -1;
  return maps * static_cast<long long>(sizeof(int));
}

extern "C" int posu_decode_views(const float* const* outputs, const float* const* flipped, const int* perm, int shift,
                                 const float* const* targets, const double* affine64, int V, int N, int J, int H,
                                 int W, int post_process, double thr, float* merged_out, float* preds_out,
                                 long long row0, long long rows, double* acc, double* avg, int* cnt, double* step,
                                 void* workspace, long long workspace_bytes, void* stream) {
  POSU_REQUIRE(V >= 1 && V <= kMaxViews, "posu_decode_views: 1 to 8 views");
  POSU_REQUIRE(N >= 0 && J > 0 && H > 0 && W > 0 && static_cast<long long>(H) * W < (1LL << 31),
               "posu_decode_views: bad shape");
  const long long need = posu_decode_views_workspace(V, N, J);
  POSU_REQUIRE(need >= 0, "posu_decode_views: shape too large");
  POSU_REQUIRE(row0 >= 0 && rows >= 0 && row0 <= rows && static_cast<long long>(V) * N <= rows - row0,
               "posu_decode_views: rows [row0, row0 + V * N) do not fit the output buffers");
  if (N == 0) return POSU_OK;  // nothing to read or write: empty tensors have no address
  POSU_REQUIRE(outputs && preds_out, "posu_decode_views: null pointer");
  DecodeViews views = {};
  for (int v = 0; v < V; ++v) {
    POSU_REQUIRE(outputs[v] && (!flipped || flipped[v]) && (!targets || targets[v]),
                 "posu_decode_views: null view pointer");
    POSU_REQUIRE(merged_out != outputs[v] && (!flipped || merged_out != flipped[v]),
                 "posu_decode_views: merged_out must not alias an input");
    views.out[v] = outputs[v];
    views.flip[v] = flipped ? flipped[v] : nullptr;
    views.tgt[v] = targets ? targets[v] : nullptr;
  }
  if (targets) {
    POSU_REQUIRE(acc && avg && cnt && step && workspace,
                 "posu_decode_views: null pointer (targets need acc, avg, cnt, step and a workspace)");
    POSU_REQUIRE(workspace_bytes >= need, "posu_decode_views: workspace too small");
    POSU_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                 "posu_decode_views: workspace must be 4-byte aligned");
    POSU_REQUIRE(((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(avg) |
                   reinterpret_cast<uintptr_t>(step)) & 7) == 0,
                 "posu_decode_views: acc, avg and step must be 8-byte aligned");
  }
  POSU_REQUIRE((reinterpret_cast<uintptr_t>(affine64) & 7) == 0, "posu_decode_views: affine64 must be 8-byte aligned");
  hipStream_t s = as_stream(stream);
  int* flags = static_cast<int*>(workspace);
  hipLaunchKernelGGL(decode_views_kernel, dim3(static_cast<unsigned>(V) * N * J), dim3(64), 0, s, views, perm, V, N,
                     J, H, W, shift, post_process, affine64, thr, row0, merged_out, preds_out, flags);
  if (targets) {
    hipLaunchKernelGGL(pck_view_kernel, dim3(V), dim3(64), 0, s, flags, N, J, acc, avg, cnt);
    hipLaunchKernelGGL(pck_step_kernel, dim3(1), dim3(64), 0, s, avg, cnt, V, step);
  }
  return check_launch("posu_decode_views");
}

extern "C" int posu_detection_counts(const float* pred, int pred_stride, const double* gt, const double* head,
                                     const unsigned char* vis, const double* thresholds, int T, int form, int N,
                                     int J, int* counts, void* stream) {
  POSU_REQUIRE(counts && thresholds, "posu_detection_counts: null pointer");
  POSU_REQUIRE(T >= 1 && T <= kMaxDetThre, "posu_detection_counts: 1 to 8 thresholds");
  POSU_REQUIRE(N >= 0 && J > 0 && static_cast<long long>(N) * J * 3 <= 0x7fffffffLL,
               "posu_detection_counts: bad shape");
  POSU_REQUIRE(pred_stride == 2 || pred_stride == 3, "posu_detection_counts: pred is [N, J, 2] or [N, J, 3]");
  POSU_REQUIRE(form == 0 || form == 1, "posu_detection_counts: form 0 (d <= head * thr) or 1 (d / head <= thr)");
  POSU_REQUIRE(N == 0 || (pred && gt && head), "posu_detection_counts: null pointer");
  DetThresholds th;
  for (int t = 0; t < kMaxDetThre; ++t) th.v[t] = t < T ? thresholds[t] : 0.0;
  const size_t bytes = static_cast<size_t>(T) * 2 * J * sizeof(int);
  const hipError_t e = hipMemsetAsync(counts, 0, bytes, as_stream(stream));
  if (e != hipSuccess) {
    set_error(std::string("posu_detection_counts: ") + hipGetErrorString(e));
    return POSU_ERR_HIP;
  }
  if (N == 0) return POSU_OK;
  hipLaunchKernelGGL(detection_counts_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), pred, pred_stride,
                     gt, head, vis, th, T, form, N, J, counts);
  return check_launch("posu_detection_counts");
}
