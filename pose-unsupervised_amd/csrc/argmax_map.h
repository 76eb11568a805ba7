// The argmax of one heatmap by one wave64 (get_max_preds, lib/core/inference.py:19-47), shared by
// posu_argmax2d_fwd (heatmap.hip), posu_pck_accuracy (train_metrics.hip) and posu_decode_views
// (validate.hip).
#pragma once
#include "posu_common.h"

namespace posu {

// The lanes' (best, bidx) pairs -> the wave's on every lane: the larger value, the smaller index on a
// tie.  A lane that met no element holds (-inf, 0x7fffffff).
__device__ __forceinline__ void wave_argmax_lanes(float& best, int& bidx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bidx, o, 64);
    if (ov > best || (ov == best && oi < bidx)) {
      best = ov;
      bidx = oi;
    }
  }
}

// best / bidx on every lane: the maximum of h[0 .. HW) and its first (smallest) index; bidx =
// 0x7fffffff when no element compares greater than -inf (an all -inf / NaN map).
// kVec4: 16-B loads when HW is a multiple of 4 and the map is 16-B aligned (a view with a storage
// offset that is not a multiple of 4 floats takes the 4-B loop).  A lane meets its elements in
// rising index order either way and ties between lanes go to the smaller index, so both loops give
// the same (best, bidx).
template <bool kVec4>
__device__ __forceinline__ void wave_argmax(const float* __restrict__ h, int HW, int lane, float& best, int& bidx) {
  best = -INFINITY;
  bidx = 0x7fffffff;
  auto take = [&](float v, int i) {
    if (v > best) {  // strict: the first (smallest) index of a tie within the lane
      best = v;
      bidx = i;
    }
  };
  if (kVec4 && (HW & 3) == 0 && (reinterpret_cast<size_t>(h) & 15) == 0) {
    const float4* h4 = reinterpret_cast<const float4*>(h);
    for (int i = lane; i < HW / 4; i += 64) {
      const float4 v = h4[i];
      take(v.x, 4 * i);
      take(v.y, 4 * i + 1);
      take(v.z, 4 * i + 2);
      take(v.w, 4 * i + 3);
    }
  } else {
    for (int i = lane; i < HW; i += 64) take(h[i], i);
  }
  wave_argmax_lanes(best, bidx);
}

// (x, y) = (idx % W, floor(idx / W)), zeroed when maxval <= 0 (inference.py:38-45)
__device__ __forceinline__ void argmax_coords(float best, int bidx, int W, float& px, float& py) {
  if (bidx == 0x7fffffff) bidx = 0;  // all -inf / NaN map
  px = static_cast<float>(bidx % W);
  py = floorf(static_cast<float>(bidx) / W);
  if (!(best > 0.f)) {
    px = 0.f;
    py = 0.f;
  }
}

}  // namespace posu
