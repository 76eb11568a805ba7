// Tail of the FIRST Bottleneck of layer2 (lib/models/pose_resnet.py:61-99 with the downsample
// branch, pose_resnet.py:136-141; eval mode, BN folded) of PoseResNet at 256x256:
//
//     y = relu( [w3*s3 | wd*sd] . [ relu(bn2(conv2_3x3_s2(t1))) ; x(2 oy, 2 ox) ] + (b3 + bd) )
//
// t1 [N, H, 64, 128] (conv1's output), x [N, H, 64, 256] (the block input), y [N, H/2, 32, 512].
// The plan ran this as two launches: the 3x3 / stride-2 conv2 (reading t1 with a 1.74x over-fetch
// of its overlapping windows, writing t2) and the two-source 1x1 "dual" GEMM (t2 plus the stride-2
// pixels of x); here t2 never leaves the CU and t1 is read once per tile window.
//
// One workgroup (4 waves, two workgroups per CU) owns 4 output rows x 16 output columns = 64 px:
//   LDS   the t1 window (rows 2 R0 - 1 .. 2 R0 + 7, columns 2 C0 - 1 .. 2 C0 + 31, zeros outside
//         the image = conv2's padding; 9 x 33 px x 256 B, LDS-DMA), BN2; after conv2, over the
//         window: t2 [64 px][128 ch], the tile's stride-2 x pixels [64 px][256 ch] (LDS-DMA) and
//         the shift b3 + bd.
//   wave  cq owns conv2 output channels 32 cq .. + 31 (2 n-tiles) and, in dual chunk nc, output
//         channels 128 nc + 32 cq .. + 31; its 4 m-tiles are the tile's 4 output rows (16 px each).
//   weights  streamed from L2 straight into VGPRs kD k-steps ahead (one contiguous 2 KB per
//         k-step and wave, packing.pack_s2_tail_stream): conv2 tap t, channel step d (k-step
//         4 t + d: conv_igemm's tap-major K order), then per dual chunk its 12 k-steps (t2's 4,
//         then x's 8: the dual GEMM's K order) -- the same MFMA sequence per accumulator as the
//         two launches, so t2 and y are bit-identical to them.
// LDS images are [pixel][channels] rows with the 16-B chunk index XOR (LDS column & 15): the
// stride-2 window reads of a 16-lane group (columns 2 r + dx) and the stride-1 t2 / x reads then
// hit 16 distinct chunk slots.
// FRONT (posu_bottleneck_s2_front_tail[_next]_fwd): t1 is not read but computed -- the block's conv1
// + BN1 + ReLU over the tile's window from x, into the same LDS image -- so the block is one launch
// (the FRONT block in the kernel says how).
// MFMA operands swapped (A = weights, B = pixels): lane (r16, q) accumulates channels 4q .. 4q+3
// of pixel r16; v_permlane16_swap pairs the 2 n-tiles into 8 consecutive channels.
#include "tail_common.h"

namespace posu {
namespace {

template <bool NEXT, bool FRONT = false>
struct S2Cfg {
  static constexpr int kWin = 64, kC = 256, kP = 128, kCout = 512, kWout = 32;
  static constexpr int kRows = 4, kTW = 16, kNW = 4, kPx = kRows * kTW;   // 64 output px
  static constexpr int kWR = 2 * kRows + 1, kWC = 2 * kTW + 1;            // 9 x 33 window
  static constexpr int kRowB = kP * 2;                                    // 256 B per t1 / t2 pixel
  static constexpr int kXRowB = kC * 2;                                   // 512 B per x pixel
  static constexpr int kWinInst = (kWR * kWC * kRowB + 1023) / 1024;      // 1 KB DMA instructions
  static constexpr int kBN2 = kWinInst * 1024;                            // s2 b2 behind the window
  static constexpr int kLds = kBN2 + 2 * kP * 4;
  static constexpr int kT2 = 0;                                           // after conv2, over the window
  static constexpr int kX = kT2 + kPx * kRowB;
  static constexpr int kShift = kX + kPx * kXRowB;
  static constexpr int kKT = kP / 32;                                     // k-steps per tap / over t2
  static constexpr int kKX = kC / 32;                                     // k-steps over x
  static constexpr int kNC = kCout / (32 * kNW);                          // dual chunks of 128 channels
  // NEXT: after each dual chunk, the next conv1's kKT k-steps over that chunk's 128 y channels
  static constexpr int kSteps2 = 9 * kKT, kStepsC = kKT + kKX + (NEXT ? kKT : 0);
  // FRONT: this block's conv1 (kKX k-steps over x) in front of conv2's; kWinPx: the window's
  // capacity in pixels, kGroups: conv1's pixel groups of kRows m-tiles over it
  static constexpr int kF = FRONT ? kKX : 0;
  static constexpr int kWinPx = kWinInst * 1024 / kRowB, kGroups = (kWR * kWC + 16 * kRows - 1) / (16 * kRows);
  static constexpr int kSteps = kF + kSteps2 + kNC * kStepsC;             // 36 + 4 x 12 = 84 (NEXT: 100; FRONT: + 8)
  static constexpr int kYC = kShift + kCout * 4;                          // NEXT: the y chunk [64 px][128 ch]
  static constexpr int kD = 4;                                            // weight prefetch depth (k-steps)
  static_assert(kYC + (NEXT ? kPx * kRowB : 0) <= kBN2, "t2, the x pixels, the shift (and the y chunk) fit over the window");
  static_assert(2 * kLds <= 160 * 1024, "two workgroups per CU");
  static_assert(kKT % kD == 0 && kKX % kD == 0 && kSteps2 % kD == 0 && kStepsC % kD == 0 && kF % kD == 0,
                "every block starts on ring slot 0");
};

// FRONT: conv1's k-steps held in registers, handed to kblock in the weight stream's place
template <int KX>
struct HeldW {
  static constexpr int kD = KX;
  uint4 wa[KX][2];
  __device__ __forceinline__ void refill(int, int) {}
};
// logical 8-channel chunk c8 of window pixel `pix` (column wc) in the swizzled window image
template <int RowB>
__device__ __forceinline__ uint4* win_chunk(char* img, int pix, int wc, int c8) {
  return reinterpret_cast<uint4*>(img + pix * RowB + ((c8 ^ (wc & 15)) << 4));
}

template <typename T, bool NEXT, bool FRONT = false>
__global__ __launch_bounds__(S2Cfg<NEXT>::kNW * 64, 2) void tail_s2_kernel(TailGeom g) {
  using O = Op<T>;
  using K = S2Cfg<NEXT, FRONT>;
  constexpr int ES = 2, MT = K::kRows;
  __shared__ __attribute__((aligned(16))) char smem[K::kLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int r16 = lane & 15, q = lane >> 4;
  const int cq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) char*)smem));
  const int Hin = g.H, Hout = Hin / 2;
  const int tiles_x = K::kWout / K::kTW, tiles_y = Hout / K::kRows;
  const int n = blockIdx.x / (tiles_x * tiles_y);
  const int rem = blockIdx.x - n * tiles_x * tiles_y;
  const int R0 = (rem / tiles_x) * K::kRows, C0 = (rem % tiles_x) * K::kTW;
  float* bn2 = reinterpret_cast<float*>(smem + K::kBN2);
  for (int c = tid; c < K::kP; c += K::kNW * 64) {
    bn2[c] = g.s2[c];
    bn2[K::kP + c] = g.b2[c];
  }

  // ---- the t1 window: 4 px per 1 KB wave-instruction, instruction m by wave m & 3
  if constexpr (!FRONT) {
    const u32x4 t1s = make_srd(g.t1, g.N * Hin * K::kWin * K::kP * ES);
    const int sub = lane >> 4, pc = lane & 15;
#pragma unroll
    for (int k = 0; k < (K::kWinInst + K::kNW - 1) / K::kNW; ++k) {
      const int m = cq + K::kNW * k;
      if (m < K::kWinInst) {  // wave-uniform
        const int pix = 4 * m + sub;
        const int wr = pix / K::kWC, wc = pix - wr * K::kWC;
        const int yy = 2 * R0 - 1 + wr, xx = 2 * C0 - 1 + wc;
        const int lc = pc ^ (wc & 15);
        const bool ok = wr < K::kWR && static_cast<unsigned>(yy) < static_cast<unsigned>(Hin) &&
                        static_cast<unsigned>(xx) < static_cast<unsigned>(K::kWin);
        dma16(t1s, ok ? (((n * Hin + yy) * K::kWin + xx) * K::kP + 8 * lc) * ES : kOOB,
              lds0 + static_cast<unsigned>(m) * 1024u);
      }
    }
  }

  // ---- the weight stream of channel group cq; the window (LDS-DMA) and the first fragments
  WStream<K::kD, K::kSteps> ws(g.wst, cq, lane);
  if constexpr (!FRONT) ws.start(g, K::kNW * 64);

  f32x4 acc[MT][2];
  f32x4 acc1[MT][2];  // NEXT: the next conv1's accumulators over the whole chunk loop
  const int c32 = 32 * cq + cpair(q);   // this lane's 8 channels of the wave's 32

  using Win = Stride2Addr<K::kRowB, K::kWC>;
  using T2 = RowsAddr<K::kRowB, K::kTW, K::kTW>;    // t2 and the y chunk: [64 px][128 ch]
  using XI = RowsAddr<K::kXRowB, K::kTW, K::kTW>;   // the stride-2 x pixels: [64 px][256 ch]

  // ---- FRONT: t1 = relu(bn1(conv1(x))) over the window, computed here instead of read.  The window's
  // 297 pixels (and the 3 pad pixels) are 5 groups of 64 (the last 44); a group's x pixels [64 px]
  // [256 ch] are LDS-DMA'd, each pixel once per workgroup and whole 128-B lines per access, into one
  // of two 32 KB buffers that lie in the window's own space below the last group's t1 -- laid out and
  // read like the dual GEMM's x pixels (XI) -- one group ahead of conv1's 8 k-steps over it.  Wave cq
  // computes its 32 channels of the group's 4 m-tiles with conv1's weights (the front of the stream)
  // held in registers.  The last group (taken first) is written to the window at once; the others'
  // t1 stays in registers (16 per group) until both buffers are dead.  Pixels outside the image load
  // zeros and are STORED as zeros: they are conv2's padding, and relu(b1) is not zero.  The k order
  // per accumulator, bn_relu and store_vals are the conv launch's: t1 is bit-identical to it.
  if constexpr (FRONT) {
    constexpr int kGrpPx = 16 * MT, kGrpB = kGrpPx * K::kXRowB;   // 64 px, 32 KB
    constexpr int kDma = kGrpB / 1024 / K::kNW;                   // a wave's DMA instructions per group
    static_assert(2 * kGrpB <= (K::kGroups - 1) * kGrpPx * K::kRowB, "both buffers below the last group's t1");
    static_assert(K::kGroups * kGrpPx >= K::kWinPx, "the groups cover the window");
    unsigned wv[kWarmLoads];
    warm_issue(wv, g.wst, g.wseg, g.warm, K::kNW * 64);
    HeldW<K::kKX> w1;
#pragma unroll
    for (int d = 0; d < K::kKX; ++d)
#pragma unroll
      for (int j = 0; j < 2; ++j) w1.wa[d][j] = *ws.frag(d, j);
    float sc[8], sh[8];
    ld8(g.s1 + c32, sc);
    ld8(g.b1 + c32, sh);
    const u32x4 xs = make_srd(g.x, g.N * Hin * K::kWin * K::kC * ES);
    // window pixel -> its byte offset in x (kOOB outside the image / the window) and its column
    auto px_off = [&](int pix, int& wc) {
      const int wr = pix / K::kWC;
      wc = pix - wr * K::kWC;
      const int yy = 2 * R0 - 1 + wr, xx = 2 * C0 - 1 + wc;
      const bool ok = wr < K::kWR && static_cast<unsigned>(yy) < static_cast<unsigned>(Hin) &&
                      static_cast<unsigned>(xx) < static_cast<unsigned>(K::kWin);
      return ok ? ((n * Hin + yy) * K::kWin + xx) * K::kC * ES : kOOB;
    };
    // group gr's pixels into buffer b: 2 px per 1 KB wave-instruction, instruction m by wave m & 3
    auto stage = [&](int gr, int b) {
      const int sub = lane >> 5, pc = lane & 31;
#pragma unroll
      for (int k = 0; k < kDma; ++k) {
        const int m = cq + K::kNW * k;
        const int px = 2 * m + sub, r = px & 15;
        const int lc = (pc & 16) | ((pc ^ r) & 15);
        int wc;
        const int off = px_off(kGrpPx * gr + px, wc);
        dma16(xs, off == kOOB ? kOOB : off + 8 * lc * ES, lds0 + static_cast<unsigned>(b * kGrpB + m * 1024));
      }
    };
    // every load the compiler counts is retired before the first DMA, so none of its waits -- which do
    // not count the DMA -- drains a group in flight
    warm_use(wv);
#pragma unroll
    for (int d = 0; d < K::kKX; ++d) asm volatile("" ::"v"(w1.wa[d][0].x), "v"(w1.wa[d][1].x));
    asm volatile("" ::"v"(sc[0]), "v"(sc[4]), "v"(sh[0]), "v"(sh[4]));
    stage(K::kGroups - 1, 0);
    stage(K::kGroups - 2, 1);
    uint4 held[K::kGroups][MT];
#pragma unroll
    for (int s = 0; s < K::kGroups; ++s) {
      const int gr = K::kGroups - 1 - s;   // the last group first: its t1 lies above both buffers
      if (s + 1 < K::kGroups) vm_wait<kDma>();   // group gr has landed, the next one may be in flight
      else vm_wait<0>();
      lds_barrier();
      zero(acc);
      kblock<O, K::kKX, 2>(acc, w1, 0, XI(smem + (s & 1) * kGrpB, r16, r16, q));
      lds_barrier();   // every wave is done reading the buffer
      if (s + 2 < K::kGroups) stage(gr - 2, s & 1);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        float v[8];
        pair(acc, i, v);
        bn_relu(v, sc, sh, nullptr);
        int wc;
        const bool pad = px_off(kGrpPx * gr + 16 * i + r16, wc) == kOOB;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = pad ? 0.f : v[e];
        held[s][i] = O::store_vals(v);
      }
      if (s == 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const int pix = kGrpPx * gr + 16 * i + r16;   // past the window's capacity: BN2 lies there
          if (pix < K::kWinPx) *win_chunk<K::kRowB>(smem, pix, pix % K::kWC, c32 >> 3) = held[s][i];
        }
      }
    }
    // conv2's first k-steps; the other groups' t1 over the buffers (the loop's last barrier: no wave
    // reads them any more); the window and BN2 published
#pragma unroll
    for (int d = 0; d < K::kD; ++d) ws.refill(d, K::kF + d);
#pragma unroll
    for (int s = 1; s < K::kGroups; ++s)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int pix = kGrpPx * (K::kGroups - 1 - s) + 16 * i + r16;
        *win_chunk<K::kRowB>(smem, pix, pix % K::kWC, c32 >> 3) = held[s][i];
      }
    vm_wait<0>();
    lds_barrier();
  }

  // ---- conv2: 9 taps x 4 channel steps; m-tile i = output row i: window row 2 i + dy, column
  // 2 r16 + dx
  zero(acc);
#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    const int dy = t / 3, dx = t - 3 * (t / 3);
    kblock<O, K::kKT, 2>(acc, ws, K::kF + K::kKT * t, Win(smem, dy, dx, r16, q));
  }
  // every wave is done reading the window: the tile's stride-2 x pixels are DMA'd over it while
  // BN2 + ReLU write t2 beside them
  lds_barrier();
  {
    const u32x4 xs = make_srd(g.x, g.N * Hin * K::kWin * K::kC * ES);
    const int sub = lane >> 5, pc = lane & 31;
#pragma unroll
    for (int k = 0; k < K::kPx / 2 / K::kNW; ++k) {
      const int m = cq + K::kNW * k;
      const int px = 2 * m + sub, i = px >> 4, r = px & 15;
      const int lc = (pc & 16) | ((pc ^ r) & 15);
      dma16(xs, (((n * Hin + 2 * (R0 + i)) * K::kWin + 2 * (C0 + r)) * K::kC + 8 * lc) * ES,
            lds0 + static_cast<unsigned>(K::kX + m * 1024));
    }
  }
  {
    float* shl = reinterpret_cast<float*>(smem + K::kShift);
    for (int c = tid; c < K::kCout; c += K::kNW * 64) shl[c] = g.b3[c];
    float sc[8], sh[8];
    ld8(bn2 + c32, sc);
    ld8(bn2 + K::kP + c32, sh);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v[8];
      pair(acc, i, v);
      bn_relu(v, sc, sh, nullptr);
      lds_store8<O, K::kRowB>(smem + K::kT2, 16 * i + r16, r16, c32 >> 3, v);
    }
  }
  vm_wait<0>();  // the x DMA (and the weight prefetches)
  lds_barrier();

  // ---- the dual GEMM, chunk nc: output channels 128 nc + 32 cq ..; K = t2's 128 channels, then
  // the 256 channels of x (2 oy, 2 ox)
  const float* shl = reinterpret_cast<const float*>(smem + K::kShift);
  T* yg = reinterpret_cast<T*>(g.y);
  if constexpr (NEXT) zero(acc1);
#pragma unroll
  for (int nc = 0; nc < K::kNC; ++nc) {
    const int p0 = K::kF + K::kSteps2 + K::kStepsC * nc;
    zero(acc);
    kblock<O, K::kKT, 2>(acc, ws, p0, T2(smem + K::kT2, r16, r16, q));
    kblock<O, K::kKX, 2>(acc, ws, p0 + K::kKT, XI(smem + K::kX, r16, r16, q));
    const int c0 = 128 * nc + c32;
    float sh[8];
    ld8(shl + c0, sh);
    if constexpr (NEXT) {
      if (nc > 0) lds_barrier();  // every wave is done reading the previous y chunk
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v[8];
      pair(acc, i, v);
      add8<false>(v, sh);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
      const size_t pix = (static_cast<size_t>(n) * Hout + R0 + i) * K::kWout + C0 + r16;
      *reinterpret_cast<uint4*>(yg + pix * K::kCout + c0) = O::store_vals(v);
      // NEXT: the chunk's y (the rounded values just stored), laid out like t2
      if constexpr (NEXT) lds_store8<O, K::kRowB>(smem + K::kYC, 16 * i + r16, r16, c32 >> 3, v);
    }
    if constexpr (NEXT) {
      // the next block's conv1 over this K slice (y channels 128 nc ..): the k order of a conv
      // launch over y, so t1n is bit-identical to it
      lds_barrier();
      kblock<O, K::kKT, 2>(acc1, ws, p0 + K::kKT + K::kKX, T2(smem + K::kYC, r16, r16, q));
    }
  }
  if constexpr (NEXT) {
    // t1n = relu(conv1n * s1n + b1n): this lane's 8 channels of each m-tile's pixel
    T* tg = reinterpret_cast<T*>(g.t1n);
    float sc[8], sh[8];
    ld8(g.s1n + c32, sc);
    ld8(g.b1n + c32, sh);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v[8];
      pair(acc1, i, v);
      bn_relu(v, sc, sh, nullptr);
      const size_t pix = (static_cast<size_t>(n) * Hout + R0 + i) * K::kWout + C0 + r16;
      *reinterpret_cast<uint4*>(tg + pix * K::kP + c32) = O::store_vals(v);
    }
  }
}

}  // namespace
}  // namespace posu

using namespace posu;

namespace {
template <typename T>
void s2_launch(bool next, bool front, dim3 grid, dim3 block, hipStream_t s, const TailGeom& g) {
  if (front) {
    if (next) hipLaunchKernelGGL((tail_s2_kernel<T, true, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((tail_s2_kernel<T, false, true>), grid, block, 0, s, g);
  } else {
    if (next) hipLaunchKernelGGL((tail_s2_kernel<T, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((tail_s2_kernel<T, false>), grid, block, 0, s, g);
  }
}

// front: conv1 inside the tail (t1 = nullptr, its BN s1 / b1, its k-steps in front of the stream)
int s2_tail_impl(const char* name, int dtype, bool front, const void* t1, const float* s1, const float* b1,
                 const void* x, int N, int H, int W, int C, int P, const void* wstream, long long wstream_bytes,
                 const float* s2, const float* b2, const float* shift, int Cout, void* y, const float* s1n,
                 const float* b1n, void* t1n, void* stream) {
  const std::string what = name;
  const bool next = t1n != nullptr;
  using K = S2Cfg<false>;
  POSU_REQUIRE(dtype == POSU_BF16 || dtype == POSU_F16, what + ": dtype must be BF16 or F16");
  TailGeom g;
  if (int e = tail_operands(g, what, t1, x, N, H, wstream, wstream_bytes, s2, b2, nullptr, shift, y, s1n, b1n, t1n,
                            front, s1, b1))
    return e;
  POSU_REQUIRE(W == K::kWin && C == K::kC && P == K::kP && Cout == K::kCout,
               what + ": built for the first Bottleneck of layer2 of PoseResNet at 256x256 (input W = 64, C = 256, "
                      "planes = 128, output channels 512)");
  const int steps = (next ? S2Cfg<true>::kSteps : K::kSteps) + (front ? S2Cfg<false, true>::kF : 0);
  const long long need = static_cast<long long>(K::kNW) * steps * 2 * 1024;
  if (int e = tail_sizes(g, what, 2 * K::kRows, static_cast<long long>(N) * H * W * C * 2, wstream_bytes, need))
    return e;
  const dim3 grid(static_cast<unsigned>(N * (H / 2 / K::kRows) * (K::kWout / K::kTW)));
  hipStream_t s = as_stream(stream);
  if (dtype == POSU_BF16) s2_launch<uint16_t>(next, front, grid, dim3(K::kNW * 64), s, g);
  else s2_launch<f16_t>(next, front, grid, dim3(K::kNW * 64), s, g);
  return check_launch(name);
}
}  // namespace

// The tail of the first Bottleneck of layer2 (see the top of this file).  wstream =
// packing.pack_s2_tail_stream(conv2 pack [128][1152], dual pack [512][384]); wstream_bytes its size.
extern "C" int posu_bottleneck_s2_tail_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C,
                                           int P, const void* wstream, long long wstream_bytes, const float* s2,
                                           const float* b2, const float* shift, int Cout, void* y, void* stream) {
  return s2_tail_impl("posu_bottleneck_s2_tail_fwd", dtype, false, t1, nullptr, nullptr, x, N, H, W, C, P, wstream,
                      wstream_bytes, s2, b2, shift, Cout, y, nullptr, nullptr, nullptr, stream);
}

// The same, chained with the next (identity) block's conv1 + BN1 + ReLU over y, like
// posu_bottleneck_tail_stream_next_fwd: t1n [N][H/2][32][128] is bit-identical to a conv launch
// over y, and that block skips its conv1 launch.  wstream = packing.pack_s2_tail_stream(conv2
// pack, dual pack, next conv1 pack [128][512]).
extern "C" int posu_bottleneck_s2_tail_next_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C,
                                                int P, const void* wstream, long long wstream_bytes, const float* s2,
                                                const float* b2, const float* shift, int Cout, void* y,
                                                const float* s1n, const float* b1n, void* t1n, void* stream) {
  if (!t1n) {
    set_error("posu_bottleneck_s2_tail_next_fwd: null pointer (t1n)");
    return POSU_ERR_ARG;
  }
  return s2_tail_impl("posu_bottleneck_s2_tail_next_fwd", dtype, false, t1, nullptr, nullptr, x, N, H, W, C, P,
                      wstream, wstream_bytes, s2, b2, shift, Cout, y, s1n, b1n, t1n, stream);
}

// The whole first Bottleneck of layer2 in one launch: conv1 + BN1 + ReLU (s1, b1 [128] f32) computed
// on each tile's window from x, then the tail above; y is bit-identical to the conv1 launch followed
// by posu_bottleneck_s2_tail_fwd.  wstream = packing.pack_s2_tail_stream(conv2 pack, dual pack,
// w1=conv1 pack [128][256]): conv1's 8 k-steps in front.
extern "C" int posu_bottleneck_s2_front_tail_fwd(int dtype, const void* x, int N, int H, int W, int C, int P,
                                                 const float* s1, const float* b1, const void* wstream,
                                                 long long wstream_bytes, const float* s2, const float* b2,
                                                 const float* shift, int Cout, void* y, void* stream) {
  return s2_tail_impl("posu_bottleneck_s2_front_tail_fwd", dtype, true, nullptr, s1, b1, x, N, H, W, C, P, wstream,
                      wstream_bytes, s2, b2, shift, Cout, y, nullptr, nullptr, nullptr, stream);
}

// The same, chained with the next block's conv1 like posu_bottleneck_s2_tail_next_fwd (wstream: +
// the next conv1 pack).
extern "C" int posu_bottleneck_s2_front_tail_next_fwd(int dtype, const void* x, int N, int H, int W, int C, int P,
                                                      const float* s1, const float* b1, const void* wstream,
                                                      long long wstream_bytes, const float* s2, const float* b2,
                                                      const float* shift, int Cout, void* y, const float* s1n,
                                                      const float* b1n, void* t1n, void* stream) {
  if (!t1n) {
    set_error("posu_bottleneck_s2_front_tail_next_fwd: null pointer (t1n)");
    return POSU_ERR_ARG;
  }
  return s2_tail_impl("posu_bottleneck_s2_front_tail_next_fwd", dtype, true, nullptr, s1, b1, x, N, H, W, C, P,
                      wstream, wstream_bytes, s2, b2, shift, Cout, y, s1n, b1n, t1n, stream);
}
