// What the register-streamed Bottleneck tails (tail_stream.hip, tail_s2.hip) share: the per-wave
// weight stream, the k-step block over a swizzled LDS image with its address functors, the
// accumulator pairing and epilogue arithmetic, and the host-side operand checks.  gfx950 only.
#pragma once
#include <string>

#include "gemm_common.h"

namespace posu {
namespace {

struct TailGeom {
  const void* t1;
  const void* x;
  void* y;
  const uint4* wst;  // [channel groups][k-steps][2 n-tiles][64 lanes] x 16 B
  const float* s2;
  const float* b2;
  const float* s3;   // (the strided tail: nullptr, its scales are folded into the weights)
  const float* b3;   // (the strided tail: b3 + bd)
  int N, H;
  // NEXT (chained tails): the next block's conv1 + BN1 + ReLU computed from this block's output y
  // while it is produced (t1n = relu(y conv1n * s1n + b1n))
  const float* s1n;
  const float* b1n;
  void* t1n;
  long long wseg;  // the weight stream's 64-B segments (warm-up, gemm_common.h)
  int warm;        // warm-up workgroups (0: none)
  // FRONT (the strided tail): this block's own conv1 + BN1 + ReLU computed from x (t1 = nullptr)
  const float* s1;
  const float* b1;
};

// ---- the weight stream of one wave: fragment j (n-tile j of the wave's 32 output channels) of k-step
// p, one contiguous 2 KB per k-step and wave, held kD k-steps ahead of their use in a register ring
// (k-step p in slot p % kD); prefetches past the end reload the last k-step
template <int D, int STEPS>
struct WStream {
  static constexpr int kD = D;
  const char* grp;  // the wave's channel group (wave-uniform)
  int wlane;
  uint4 wa[D][2];
  __device__ __forceinline__ WStream(const uint4* wst, int cq, int lane)
      : grp(reinterpret_cast<const char*>(wst) + cq * (STEPS * 2 * 1024)), wlane(lane * 16) {}
  __device__ __forceinline__ const uint4* frag(int p, int j) const {
    return reinterpret_cast<const uint4*>(grp + (min(p, STEPS - 1) * 2 + j) * 1024 + wlane);
  }
  __device__ __forceinline__ void refill(int slot, int p) {
    wa[slot][0] = *frag(p, 0);
    wa[slot][1] = *frag(p, 1);
  }
  // the first kD k-steps and the stream's warm-up (gemm_common.h: every line requested up front);
  // returns once they and the LDS-DMA issued before have landed, behind a workgroup barrier
  __device__ __forceinline__ void start(const TailGeom& g, int threads) {
#pragma unroll
    for (int d = 0; d < D; ++d) refill(d, d);
    unsigned wv[kWarmLoads];
    warm_issue(wv, g.wst, g.wseg, g.warm, threads);
    vm_wait<0>();
    warm_use(wv);
    lds_barrier();
  }
};

template <int MT>
__device__ __forceinline__ void zero(f32x4 (&a)[MT][2]) {
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) a[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// MFMA operands swapped (A = weights, B = pixels): lane (r16, q) accumulates channels 4q .. 4q+3 of
// pixel r16; v_permlane16_swap pairs m-tile i's 2 n-tiles into this lane's 8 consecutive channels
// cpair(q) .. cpair(q) + 7 of the wave's 32
template <int MT>
__device__ __forceinline__ void pair(const f32x4 (&a)[MT][2], int i, float* v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(a[i][0][e]), __float_as_uint(a[i][1][e]),
                                                     false, false);
    v[e] = __uint_as_float(sw[0]);
    v[4 + e] = __uint_as_float(sw[1]);
  }
}
__device__ __forceinline__ int cpair(int q) { return 16 * (q & 1) + 8 * (q >> 1); }

// 8 consecutive f32 (16-byte aligned: BN scales / shifts at the lane's channels) as two 16-B loads
__device__ __forceinline__ void ld8(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// relu(v * sc + sh (+ r)) over a lane's 8 values; the multiply-add as an explicit fma, the conv
// epilogue's contraction: left to the compiler, the split variants' epilogues were vectorised into
// v_mul + v_pk_add (two roundings) and differed from the conv launches in the last f32 bit
__device__ __forceinline__ void bn_relu(float* v, const float* sc, const float* sh, const float* r) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = fmaxf(__builtin_fmaf(v[e], sc[e], sh[e]) + (r ? r[e] : 0.f), 0.f);
}

// ---- LDS images: [pixel][channels] rows of RowB bytes, the 16-B chunk index XOR the pixel's key =
// its column (in its image) & 15.  Keyed by the column rather than the pixel index, the key of an
// m-tile's lane is the same for every m-tile of a wave, so a k-step's fragment addresses are four
// per-block base registers plus compile-time offsets (no address arithmetic in the loop).  Keys stay
// inside a pixel row: 16 chunks or more take (column & 15), the 8-chunk rows of 64-channel 2-byte
// images (layer1 at 384x384) (column & 7).
template <int RowB>
constexpr int kKeyMask = RowB / 16 >= 16 ? 15 : RowB / 16 - 1;

// a lane's 8 values into logical 8-channel chunk c8 of pixel `pix` (split: its hi and lo chunks)
template <typename O, int RowB>
__device__ __forceinline__ void lds_store8(char* img, int pix, int key, int c8, const float* v) {
  auto at = [&](int chunk) { return reinterpret_cast<uint4*>(img + pix * RowB + ((chunk ^ (key & kKeyMask<RowB>)) << 4)); };
  if constexpr (O::SPLIT) {
    uint4 h, l;
    split8(v, h, l);
    const int ch = split_ch(8 * c8) >> 3;
    *at(ch) = h;
    *at(ch + 4) = l;
  } else {
    *at(c8) = O::store_vals(v);
  }
}

// k-step d of a block reads the lane pixel's chunk (4 d + q) ^ key = 4 ((d & 3) ^ (key >> 2)) +
// 16 (d >> 2) + (q ^ (key & 3)): four base pointers per (lane pixel, key), the k-step's 16 B at
// kb[d & 3] + (d >> 2) * 256, plus `off` pixels
template <int RowB>
struct SwzBases {
  const char* kb[4];
  __device__ __forceinline__ void set(const char* img, int pix, int key, int q) {
    key &= kKeyMask<RowB>;
    const char* lb = img + pix * RowB + ((q ^ (key & 3)) << 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) kb[k] = lb + ((k ^ (key >> 2)) << 6);
  }
  __device__ __forceinline__ const uint4* at(int d, int off) const {
    return reinterpret_cast<const uint4*>(kb[d & 3] + off * RowB + (d >> 2) * 256);
  }
};

// swizzle key of the t1 window's pixel (window row wr, column wc): the column & 15 for W a multiple
// of 16; for W = 24 the column plus 8 on odd rows, so the 16 lanes of an m-tile that straddles two
// image rows (columns 16 .. 23 of one, 0 .. 7 of the next) still hit 16 distinct chunk slots
template <int W>
__device__ __forceinline__ int wkey(int wr, int wc) {
  return W % 16 == 0 ? (wc & 15) : ((wc + 8 * (wr & 1)) & 15);
}

// Address functors of kblock: (m-tile i, k-step d) -> this lane's 16 B of the pixel operand.
// Stride 1 (the t1 window of W a multiple of 16, t2, x, the y chunk): m-tile i holds pixels 16 i ..
// of a W-wide tile, row-major, in an image of COLS pixels per row; lpix / key: m-tile 0's pixel of
// this lane and its column
template <int RowB, int W, int COLS>
struct RowsAddr {
  SwzBases<RowB> b;
  __device__ __forceinline__ RowsAddr(const char* img, int lpix, int key, int q) { b.set(img, lpix, key, q); }
  __device__ __forceinline__ const uint4* operator()(int i, int d) const {
    return b.at(d, (16 * i / W) * COLS + (16 * i) % W);
  }
};
// The W = 24 window at tap (dy, dx): m-tiles straddle image rows -- m-tile i = 3 m + c holds tile
// pixels 48 m + 16 c .. (rows 2 m, 2 m + 1), three lane-address classes c, each with its own bases,
// at + 2 m window rows
template <int RowB, int COLS>
struct Win24Addr {
  SwzBases<RowB> c[3];
  __device__ __forceinline__ Win24Addr(const char* img, int dy, int dx, int r16, int q) {
    const int bb = r16 >= 8;
    const int ro[3] = {0, bb, 1}, co[3] = {r16, 16 + r16 - 24 * bb, 8 + r16};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      c[k].set(img, (ro[k] + dy) * COLS + co[k] + dx, wkey<24>(ro[k] + dy, co[k] + dx), q);
  }
  __device__ __forceinline__ const uint4* operator()(int i, int d) const { return c[i % 3].at(d, (i / 3) * 2 * COLS); }
};
// The stride-2 window at tap (dy, dx): m-tile i = output row i, window row 2 i + dy, column 2 r16 + dx
template <int RowB, int COLS>
struct Stride2Addr {
  SwzBases<RowB> b;
  __device__ __forceinline__ Stride2Addr(const char* img, int dy, int dx, int r16, int q) {
    b.set(img, dy * COLS + 2 * r16 + dx, 2 * r16 + dx, q);
  }
  __device__ __forceinline__ const uint4* operator()(int i, int d) const { return b.at(d, 2 * i * COLS); }
};

// One block of KT k-steps (stream k-steps p0 .., p0 a multiple of kD: the ring slot of k-step d is the
// compile-time d % kD) into acc: k-step d multiplies the stream's fragments with the pixel fragments
// at(i, d) of every m-tile i.  NB = 2: the pixel fragments of k-step d + 1 are read while k-step d's
// MFMAs run (two register sets); NB = 1: m-tile i's next fragment once its MFMAs are issued.  The
// scheduling barriers keep the compiler from hoisting more of them.
// Split fp16 (O::SPLIT): the k-step pairs (2c, 2c + 1) are the hi and the lo halves of the same 32
// channels, in the weight stream too, multiplied as hi.hi + lo(w).hi(x) + hi(w).lo(x) (the conv
// kernel's order per accumulator: bit-identical to it).
template <typename O, int KT, int NB, int MT, typename WS, typename AT>
__device__ __forceinline__ void kblock(f32x4 (&acc)[MT][2], WS& ws, int p0, const AT& at) {
  constexpr int kD = WS::kD;
  uint4 b[NB][MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) b[0][i] = *at(i, 0);
#pragma unroll
  for (int d = 0; d < KT; ++d) {
    if (NB == 2 && d + 1 < KT) {
#pragma unroll
      for (int i = 0; i < MT; ++i) b[(d + 1) % NB][i] = *at(i, d + 1);
    }
    const int s = d % kD;
    if constexpr (O::SPLIT) {
      // the hi step (d even) issues both uses of its pixel fragments, hi.hi then lo(w).hi(x) (the
      // lo weights of step d + 1 are in their slot already), the lo step hi(w).lo(x); then the slot
      // used for the last time is refilled: the lo weights' after the hi step, the hi weights'
      // after the lo step (a slot keeps its k-steps mod kD)
      const int s2 = (d & 1) ? s - 1 : s + 1;
      if ((d & 1) == 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) O::mma(acc[i][j], ws.wa[s][j], b[d % NB][i]);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) O::mma(acc[i][j], ws.wa[s2][j], b[d % NB][i]);
      ws.refill(s2, p0 + ((d & 1) ? d - 1 : d + 1) + kD);
    } else {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) O::mma(acc[i][j], ws.wa[s][j], b[d % NB][i]);
        if (NB == 1 && d + 1 < KT) b[0][i] = *at(i, d + 1);
      }
      ws.refill(s, p0 + d + kD);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- host side: the operand checks of both tails' entry points.  tail_operands() before the variant
// is known (and the launch's TailGeom), tail_sizes() once it is: `hmult` the rows H must divide into,
// `act_bytes` the largest activation, `need` the bytes of the stream the variant reads.
inline int tail_operands(TailGeom& g, const std::string& what, const void* t1, const void* x, int N, int H,
                         const void* wstream, long long wstream_bytes, const float* s2, const float* b2,
                         const float* s3, const float* b3, void* y, const float* s1n, const float* b1n, void* t1n,
                         bool front = false, const float* s1 = nullptr, const float* b1 = nullptr) {
  // front: conv1 runs inside the tail -- its BN in place of its output t1
  POSU_REQUIRE((front ? s1 && b1 : t1 != nullptr) && x && wstream && s2 && b2 && b3 && y, what + ": null pointer");
  POSU_REQUIRE(x != y && t1 != y, what + ": the output must not alias an input");
  POSU_REQUIRE(!t1n || (s1n && b1n && t1n != y && t1n != x && t1n != t1),
               what + ": the next conv1 needs its BN and an output that aliases no other operand");
  g = TailGeom{t1, x, y, static_cast<const uint4*>(wstream), s2, b2, s3, b3, N, H, s1n, b1n, t1n, wstream_bytes / 64,
               warm_wgs(wstream_bytes), s1, b1};
  return POSU_OK;
}

inline int tail_sizes(const TailGeom& g, const std::string& what, int hmult, long long act_bytes,
                      long long wstream_bytes, long long need) {
  POSU_REQUIRE(wstream_bytes == need, what + ": wstream holds " + std::to_string(wstream_bytes) + " bytes, the " +
                                          (g.t1n ? "chained" : "plain") + " tail reads " + std::to_string(need));
  POSU_REQUIRE(g.N > 0 && g.H > 0 && g.H % hmult == 0,
               what + ": H must be a positive multiple of " + std::to_string(hmult) + " (the tile rows)");
  POSU_REQUIRE(act_bytes < (1LL << 31) - 256, what + ": activation exceeds the 2 GiB addressing range");
  for (const void* p : {g.t1, g.x, static_cast<const void*>(g.y), static_cast<const void*>(g.wst),
                        static_cast<const void*>(g.s3), static_cast<const void*>(g.b3),
                        static_cast<const void*>(g.t1n), static_cast<const void*>(g.s1n),
                        static_cast<const void*>(g.b1n), static_cast<const void*>(g.s1),
                        static_cast<const void*>(g.b1)})
    POSU_REQUIRE((reinterpret_cast<size_t>(p) & 15) == 0, what + ": pointers must be 16-byte aligned");
  return POSU_OK;
}

}  // namespace
}  // namespace posu
