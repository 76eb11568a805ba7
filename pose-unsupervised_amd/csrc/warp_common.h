// The crop warp's arithmetic, shared by posu_crop_warp (datapath.hip) and posu_sample_images (sample.hip).
#pragma once
#include "posu_common.h"

namespace posu {

// OpenCV 3.4's warpAffine (imgwarp.cpp: WarpAffineInvoker + remapBilinear, 8-bit) restated:
// the src -> dst matrix inverted in double; source coordinates in 1/1024-px fixed point
// (cvRound = round half to even) with the row term and the column term rounded separately,
// reduced to 1/32 px; the 4 taps weighted by the exact-integer bilinear table (sum 32768);
// (sum + 2^14) >> 15.  Border: constant 0 -- a pixel whose 2x2 footprint misses the image is 0,
// a partly covered one takes 0 for the missing taps.  No FMA contraction anywhere: every
// double is rounded like OpenCV's separate multiplies and adds.
struct WarpTaps {
  int sx, sy;     // top-left tap
  int w[4];       // weights of (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1)
  bool outside;   // the whole footprint misses the image
};

#pragma clang fp contract(off)
// taps of output pixel (x, y) under the src -> dst matrix Mi[6] in an H x W source
__device__ __forceinline__ WarpTaps warp_taps(const double* __restrict__ Mi, int x, int y, int H, int W) {
  double m0 = Mi[0], m1 = Mi[1], m2 = Mi[2], m3 = Mi[3], m4 = Mi[4], m5 = Mi[5];
  double D = m0 * m4 - m1 * m3;
  D = D != 0.0 ? 1.0 / D : 0.0;
  const double a11 = m4 * D, a22 = m0 * D;
  m0 = a11;
  m1 *= -D;
  m3 *= -D;
  m4 = a22;
  const double b1 = -m0 * m2 - m1 * m5;
  const double b2 = -m3 * m2 - m4 * m5;
  m2 = b1;
  m5 = b2;
  const int adelta = static_cast<int>(rint(m0 * x * 1024.0));
  const int bdelta = static_cast<int>(rint(m3 * x * 1024.0));
  const int X0 = static_cast<int>(rint((m1 * y + m2) * 1024.0)) + 16;
  const int Y0 = static_cast<int>(rint((m4 * y + m5) * 1024.0)) + 16;
  const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  WarpTaps t;
  t.sx = min(max(X >> 5, -32768), 32767);
  t.sy = min(max(Y >> 5, -32768), 32767);
  const int fx = X & 31, fy = Y & 31;
  t.w[0] = (32 - fy) * (32 - fx) * 32;
  t.w[1] = (32 - fy) * fx * 32;
  t.w[2] = fy * (32 - fx) * 32;
  t.w[3] = fy * fx * 32;
  t.outside = t.sx >= W || t.sx + 1 < 0 || t.sy >= H || t.sy + 1 < 0;
  return t;
}
#pragma clang fp contract(on)

// channel c of the warped pixel.  flip: the source is read mirrored (data_numpy[:, ::-1, :]): tap
// column tx reads column W - 1 - tx, the border test stays on tx.
__device__ __forceinline__ int warp_channel(const unsigned char* __restrict__ S, int H, int W, int C, int c,
                                            const WarpTaps& t, bool flip) {
  if (t.outside) return 0;
  int acc = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int tx = t.sx + (k & 1), ty = t.sy + (k >> 1);
    if (tx >= 0 && tx < W && ty >= 0 && ty < H) {
      const int col = flip ? W - 1 - tx : tx;
      acc += static_cast<int>(S[(static_cast<long long>(ty) * W + col) * C + c]) * t.w[k];
    }
  }
  const int v = (acc + (1 << 14)) >> 15;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace posu
