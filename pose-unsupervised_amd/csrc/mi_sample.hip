// Position sampling of the heatmap mutual-information loss on the device (reference
// lib/core/loss.py:646-703, which samples on the host): per image the window centre, half of the
// window's entries without replacement and a quarter as many distinct positions outside it.
//
// A counter-based sampler: row k's draw is a function of (seed, call, k) and of that row's inputs,
// never of B, the launch geometry or other rows.  The words of row k are the outputs of
// Philox4x32-10 with key (seed low, seed high) and counter (b, k, call low, call high), b = 0, 1,
// 2, ..., taken in output order (include/posu.h gives the whole stream definition).
//
// One wave per row.  The window, the permutation and the set of taken positions (window + accepted)
// live in LDS.  The 64 lanes fill 64 Philox blocks (256 words) at a time; lane 0 consumes them
// through the Fisher-Yates steps and the rejection loop, and the wave refills when they run out.
// Both loops are bounded.  A latency kernel of a few microseconds: nothing here is tuned.
#include <cmath>

#include "philox_common.h"

namespace posu {
namespace {

constexpr int kMaxP = 1024;               // window entries
constexpr int kMaxHW = 65536;             // map positions
constexpr int kLanes = 64;
constexpr int kBufWords = 4 * kLanes;     // words per refill
constexpr int kDrawsPerSlot = 64;         // outside draws per position before the deterministic fill

// trunc(v / feat + 0.5) clamped to [0, size - 1], f64 with an IEEE division; NaN gives 0
__device__ __forceinline__ int grid_coordinate(double v, double feat, int size) {
  const double t = v / feat + 0.5;
  if (!(t >= 1.0)) return 0;
  if (t >= static_cast<double>(size)) return size - 1;
  return static_cast<int>(t);
}

__device__ __forceinline__ bool test_and_set(uint32_t* bits, int pos) {
  const uint32_t m = 1u << (pos & 31);
  const uint32_t old = bits[pos >> 5];
  bits[pos >> 5] = old | m;
  return (old & m) != 0;
}

__global__ __launch_bounds__(kLanes) void k_mi_sample(const double* __restrict__ joints,
                                                      const double* __restrict__ vis, int J, int joint, double feat_w,
                                                      double feat_h, int H, int W, int radius, uint32_t seed_lo,
                                                      uint32_t seed_hi, uint32_t call_lo, uint32_t call_hi,
                                                      int* __restrict__ idx, int* __restrict__ loc) {
  __shared__ int window[kMaxP];
  __shared__ uint16_t perm[kMaxP];
  __shared__ uint32_t taken[kMaxHW / 32];
  __shared__ uint32_t words[kBufWords];
  __shared__ int outside[kMaxP / 4];
  __shared__ int state[4];   // Fisher-Yates step, accepted positions, outside draws, done

  const int k = blockIdx.x, lane = threadIdx.x;
  const int side = 2 * radius + 1, P = side * side, n_in = P / 2, n_out = P / 4, Q = n_in + n_out, HW = H * W;
  const uint32_t row = static_cast<uint32_t>(k);

  // word 0 is always consumed: the centre of an invisible joint
  const Philox first = philox4x32_10(0u, row, call_lo, call_hi, seed_lo, seed_hi);
  const size_t jrow = static_cast<size_t>(k) * J + joint;
  const int gx = grid_coordinate(joints[2 * jrow], feat_w, W);
  const int gy = grid_coordinate(joints[2 * jrow + 1], feat_h, H);
  const int centre = vis[jrow] != 0.0 ? gy * W + gx : bounded(first.c[0], HW);

  for (int w = lane; w < (HW + 31) / 32; w += kLanes) taken[w] = 0u;
  for (int e = lane; e < P; e += kLanes) {
    const int dy = e / side - radius, dx = e % side - radius;
    const int p = centre + dy * W + dx;   // the linear index is clamped: a window at a border repeats positions
    window[e] = p < 0 ? 0 : (p > HW - 1 ? HW - 1 : p);
    perm[e] = static_cast<uint16_t>(e);
  }
  if (lane == 0) state[0] = state[1] = state[2] = state[3] = 0;
  __syncthreads();
  for (int e = lane; e < P; e += kLanes) atomicOr(&taken[window[e] >> 5], 1u << (window[e] & 31));

  // words 1 ..: at most 1 + n_in + kDrawsPerSlot n_out of them, so the refill count is bounded too
  const int max_words = 1 + n_in + kDrawsPerSlot * n_out;
  const int refills = (max_words + kBufWords - 1) / kBufWords;
  for (int f = 0; f < refills; ++f) {
    const Philox b = philox4x32_10(static_cast<uint32_t>(f * kLanes + lane), row, call_lo, call_hi, seed_lo, seed_hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) words[4 * lane + i] = b.c[i];
    __syncthreads();
    if (lane == 0) {
      int t = state[0], a = state[1], d = state[2];
      int c = f == 0 ? 1 : 0;   // word 0 went to the centre
      for (; c < kBufWords && t < n_in; ++c, ++t) {
        const int j = t + bounded(words[c], P - t);
        const uint16_t pt = perm[t];
        perm[t] = perm[j];
        perm[j] = pt;
      }
      if (t == n_in) {
        for (; c < kBufWords && a < n_out && d < kDrawsPerSlot * n_out; ++c, ++d) {
          const int p = bounded(words[c], HW);
          if (!test_and_set(taken, p)) outside[a++] = p;
        }
      }
      state[0] = t, state[1] = a, state[2] = d;
      state[3] = t == n_in && (a == n_out || d == kDrawsPerSlot * n_out);
    }
    __syncthreads();
    if (state[3]) break;
  }
  // acceptance is at least 1/2 (P + P / 4 <= HW / 2), so this fill is unreachable in practice: the
  // lowest free positions in ascending order
  if (lane == 0) {
    int a = state[1];
    for (int p = 0; p < HW && a < n_out; ++p)
      if (!test_and_set(taken, p)) outside[a++] = p;
  }
  __syncthreads();

  int* out = idx + static_cast<size_t>(k) * Q;
  for (int t = lane; t < n_in; t += kLanes) out[t] = window[perm[t]];
  for (int a = lane; a < n_out; a += kLanes) out[n_in + a] = outside[a];
  if (loc && lane == 0) loc[k] = centre;
}

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" int posu_heatmap_mi_sample(const double* joints, const double* vis, int B, int J, int joint_idx,
                                      double feat_w, double feat_h, int H, int W, int radius,
                                      unsigned long long seed, unsigned long long call, int* idx, int* loc,
                                      void* stream) {
  const char* fn = "posu_heatmap_mi_sample";
  const std::string f(fn);
  POSU_REQUIRE(joints && vis && idx, f + ": null pointer");
  POSU_REQUIRE(B >= 0 && J >= 1 && H >= 1 && W >= 1, f + ": negative or empty shape");
  POSU_REQUIRE(joint_idx >= 0 && joint_idx < J, f + ": joint_idx out of range");
  POSU_REQUIRE(radius >= 1, f + ": radius must be at least 1");
  const long long side = 2ll * radius + 1, P = side * side, HW = static_cast<long long>(H) * W;
  POSU_REQUIRE(radius <= 15 && P <= kMaxP, f + ": the window holds at most 1024 entries");
  POSU_REQUIRE(HW <= kMaxHW, f + ": the map holds at most 65536 positions");
  POSU_REQUIRE(P + P / 4 <= HW / 2, f + ": window too large for the map (P + P / 4 must be at most H W / 2)");
  POSU_REQUIRE(std::isfinite(feat_w) && std::isfinite(feat_h) && feat_w > 0.0 && feat_h > 0.0,
               f + ": feat_w and feat_h must be finite and positive");
  POSU_REQUIRE(static_cast<long long>(B) * J < (1ll << 31), f + ": shape too large");
  if (B == 0) return POSU_OK;
  hipLaunchKernelGGL(k_mi_sample, dim3(static_cast<unsigned>(B)), dim3(kLanes), 0, as_stream(stream), joints, vis, J,
                     joint_idx, feat_w, feat_h, H, W, radius, static_cast<uint32_t>(seed),
                     static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(call), static_cast<uint32_t>(call >> 32),
                     idx, loc);
  return check_launch(fn);
}
