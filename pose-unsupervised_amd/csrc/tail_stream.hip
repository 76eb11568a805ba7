// Tail of an identity Bottleneck (lib/models/pose_resnet.py:79-99, eval mode, BN folded) of
// PoseResNet at 256x256 with the weights streamed straight into registers, for layer2
// (W = 32, planes 128, C = 512) and layer3 (W = 16, planes 256, C = 1024):
//
//     y = relu( bn3(conv3( relu(bn2(conv2_3x3(t1))) )) + x ),   t1 = conv1's output
//
// Why (the round-2 LDS-ring versions, removed in round 4, streamed the weights through a
// two-slot 32 KB LDS ring): so one 32 KB stage is in flight per CU and every
// stage pays a full L2 round trip -- layer3's 52 stages x ~1.5 us = its 80 us (profiles/r02).
// Here the LDS holds only activations; each wave loads its own weight fragments from L2 into
// VGPRs kD k-steps ahead of their use (one contiguous 2 KB per k-step and wave, prepacked by
// packing.pack_tail_stream), so 8 waves x kD x 2 KB are in flight and no barrier sits in the
// weight stream.
//
// One workgroup (8 waves, one per CU) owns 8 image rows (128 px at W = 16, 256 px at W = 32).
// Wave w: pixel group pg = w / NCQ (128 px = 8 m-tiles each, NPG = 8 / NCQ groups), channel
// group cq = w % NCQ (32 output channels = 2 n-tiles of conv2, and of each conv3 chunk of
// 32 NCQ channels).  The pixel operands come from LDS (8 x 1 KB ds_reads per 16 MFMAs).
//   LDS: the t1 window (rows y0-1 .. y0+8, columns -1 .. W, zero padding; staged once by
//        LDS-DMA), BN2; after conv2: t2 [8 W px][P ch] and BN3 over the window.
//   weight stream of a wave: conv2 tap t, channel step c (p = KT t + c, KT = P / 32: the conv
//        kernel's tap-major K order -- bit-identical accumulators), then conv3 chunk nc,
//        channel step c (p = 9 KT + KT nc + c).
// The stream, the k-step block and the epilogue arithmetic are tail_common.h's, shared with the
// strided tail (tail_s2.hip).  Every instance of the kernel is one row of kTail below.
#include <cstddef>
#include <utility>

#include "tail_common.h"

namespace posu {
namespace {

// ---- The variants.  kTail is the whole story: one row per kernel instance (the bf16 / f16 rows
// twice, once per element type) -- what it is built for, its tile, its register budget -- and the
// host picks the row whose key (dtype class, W, P, C, NEXT, DOWN, NX, grid) matches the launch.
//   NEXT  chained: also the next block's conv1 + BN1 + ReLU over y (a second accumulator set)
//   DOWN  (round 6, layer1's first block): the Bottleneck with a stride-1 1x1 downsample
//         (pose_resnet.py:136-141) -- no residual; each conv3 chunk also runs the downsample over the
//         block input x (P channels, staged in LDS) into the same accumulators, [w3*s3 | wd*sd] with
//         shift = b3 + bd (posu_conv1x1_dual_fwd's K order: bit-identical to it)
//   NX    the next conv1's output channels in units of P: 2 when it opens the NEXT layer (layer2 / 3 /
//         4 block 0's conv1, C -> 2 P at this map size), so the last identity block of a layer chains
//         it too -- two accumulator sets, each over the same y chunk image (round 6)
//   kd, nb  weight prefetch depth in k-steps (clipped to the k-steps of a block) and pixel-fragment
//         register sets.  4 and 2 wherever they fit: since x / y / t1n sit behind buffer descriptors
//         (round 5) the chained variants fit them too (network 2.3529 / 2.3514 vs 2.3991 / 2.3966 ms
//         with round 4's 1-deep / one set on layer2 and 2-deep / two sets on layer3, profiles/r05)
//   wgs   workgroups per CU the instance is compiled for (__launch_bounds__' second argument)
enum : unsigned { D2 = 1, DS = 2 };  // dtype class, as in conv_igemm.hip: bf16 / f16, split fp16
// layer3 at W = 16: 8-row tiles (128 px, 8 m-tiles per wave) while they give every CU a workgroup,
// else 4-row tiles (64 px, 4 m-tiles per wave): at batch 64 (BASELINE configs[1]) the 8-row grid left
// half the CUs idle (128 workgroups).  kSmallGrid rows hold while N (H / 8) < kSmallGridWGs and
// H % 4 == 0, kFullGrid rows otherwise.
enum Grid { kAnyGrid, kSmallGrid, kFullGrid };
constexpr int kSmallGridWGs = 256;
struct TailRow {
  unsigned dt;
  int W, P, C;
  int rows, nw, mt;  // image rows per workgroup, waves, m-tiles (16 px) per wave
  bool next, down;
  int nx;
  int kd, nb, wgs;
  Grid grid;
};
constexpr TailRow kTail[] = {
    // layer2 (W = 32): 4 rows x 32 px with 4 waves, two workgroups per CU, so one's conv3 epilogue
    // (residual loads, y stores) overlaps the other's MFMAs; chaining the next layer: 2-row tiles,
    // 4 m-tiles per wave, whose second accumulator set fits twice
    {D2, 32, 128, 512, 4, 4, 8, false, false, 1, 4, 2, 2, kAnyGrid},
    {D2, 32, 128, 512, 4, 4, 8, true, false, 1, 4, 2, 2, kAnyGrid},
    {D2, 32, 128, 512, 2, 4, 4, true, false, 2, 4, 2, 2, kAnyGrid},
    // layer3 (W = 16): 8 rows x 16 px with 8 waves (one workgroup per CU, 256 at batch 128), or 4 rows
    {D2, 16, 256, 1024, 8, 8, 8, false, false, 1, 4, 2, 1, kFullGrid},
    {D2, 16, 256, 1024, 8, 8, 8, true, false, 1, 4, 2, 1, kFullGrid},
    {D2, 16, 256, 1024, 4, 8, 4, false, false, 1, 4, 2, 1, kSmallGrid},
    {D2, 16, 256, 1024, 4, 8, 4, true, false, 1, 4, 2, 1, kSmallGrid},
    {D2, 16, 256, 1024, 4, 8, 4, true, false, 2, 4, 2, 1, kAnyGrid},
    // layer3 at W = 24 (R152@384, round 5): 6 rows x 24 px = 144 px, nine m-tiles per wave, one
    // fragment set and a two-deep stream -- 256 VGPRs, no spills; chained (round 6): 2 rows, three
    // m-tiles per wave (with nine the second accumulator set does not fit)
    {D2, 24, 256, 1024, 6, 8, 9, false, false, 1, 2, 1, 1, kAnyGrid},
    {D2, 24, 256, 1024, 2, 8, 3, true, false, 1, 4, 2, 1, kAnyGrid},
    // layer2 at W = 48: 2 rows x 48 px = 96 px, 6 m-tiles per wave, 4 waves
    {D2, 48, 128, 512, 2, 4, 6, false, false, 1, 4, 2, 2, kAnyGrid},
    {D2, 48, 128, 512, 2, 4, 6, true, false, 1, 4, 2, 2, kAnyGrid},
    // layer1 at W = 96 (R152@384): 2 rows x 96 px = 192 px, 6 m-tiles per wave (one image row), 4 waves
    {D2, 96, 64, 256, 2, 4, 6, false, false, 1, 4, 2, 2, kAnyGrid},
    {D2, 96, 64, 256, 2, 4, 6, true, false, 1, 4, 2, 2, kAnyGrid},
    {D2, 96, 64, 256, 2, 4, 6, false, true, 1, 4, 2, 2, kAnyGrid},
    {D2, 96, 64, 256, 2, 4, 6, true, true, 1, 4, 2, 2, kAnyGrid},
    // split fp16 (round 6): layer1 (W = 64, planes 64: 2 rows x 64 px, four waves as 2 pixel x 2 channel
    // groups), layer2 (2 rows x 32 px, four waves), layer3 (4 rows x 16 px, eight waves) -- the pairs
    // double the t1 window, so the tiles are the bf16 ones' small variants (68 / 69 / 110 KB of LDS)
    {DS, 64, 64, 256, 2, 4, 4, false, false, 1, 4, 2, 2, kAnyGrid},
    {DS, 64, 64, 256, 2, 4, 4, true, false, 1, 4, 2, 2, kAnyGrid},
    {DS, 64, 64, 256, 2, 4, 4, true, false, 2, 4, 2, 2, kAnyGrid},
    {DS, 64, 64, 256, 2, 4, 4, false, true, 1, 4, 2, 1, kAnyGrid},
    {DS, 64, 64, 256, 2, 4, 4, true, true, 1, 4, 2, 1, kAnyGrid},
    {DS, 32, 128, 512, 2, 4, 4, false, false, 1, 4, 2, 2, kAnyGrid},
    {DS, 32, 128, 512, 2, 4, 4, true, false, 1, 4, 2, 2, kAnyGrid},
    {DS, 32, 128, 512, 2, 4, 4, true, false, 2, 4, 2, 2, kAnyGrid},
    {DS, 16, 256, 1024, 4, 8, 4, false, false, 1, 4, 2, 1, kAnyGrid},
    {DS, 16, 256, 1024, 4, 8, 4, true, false, 1, 4, 2, 1, kAnyGrid},
    {DS, 16, 256, 1024, 4, 8, 4, true, false, 2, 4, 2, 1, kAnyGrid},
};
constexpr int kNTail = sizeof(kTail) / sizeof(kTail[0]);

constexpr bool same_key(const TailRow& a, const TailRow& b) {
  return (a.dt & b.dt) && a.W == b.W && a.P == b.P && a.C == b.C && a.next == b.next && a.down == b.down &&
         a.nx == b.nx && (a.grid == kAnyGrid || b.grid == kAnyGrid || a.grid == b.grid);
}
constexpr bool keys_distinct() {
  for (int i = 0; i < kNTail; ++i)
    for (int j = i + 1; j < kNTail; ++j)
      if (same_key(kTail[i], kTail[j])) return false;
  return true;
}
static_assert(keys_distinct(), "no two rows share a selection key");

// the bytes of the stream a row's instance reads: NCQ channel groups x (9 KT conv2 + NC KT conv3 [+ NC
// KT downsample] [+ NC KT NX next conv1]) k-steps x 2 n-tiles x 1 KB (packing.pack_tail_stream);
// split: KT = 2 P / 32
constexpr long long stream_bytes(const TailRow& r) {
  const int kt = (r.dt == DS ? 2 : 1) * r.P / 32, ncq = r.nw / (r.rows * r.W / (16 * r.mt)), nc = r.C / (32 * ncq);
  return static_cast<long long>(ncq) * (9 * kt + nc * kt * (1 + r.down + r.next * r.nx)) * 2 * 1024;
}

template <int R>
struct TailCfg {
  static constexpr int W = kTail[R].W, P = kTail[R].P, C = kTail[R].C, NX = kTail[R].nx;
  static constexpr bool NEXT = kTail[R].next, DOWN = kTail[R].down;
  static constexpr int kRows = kTail[R].rows;      // image rows per workgroup
  static constexpr int kNW = kTail[R].nw;          // waves per workgroup
  static constexpr int kMT = kTail[R].mt;          // m-tiles (16 px) per wave
  static constexpr int kPx = kRows * W;            // tile pixels
  static constexpr int kNPG = kPx / (16 * kMT);    // pixel groups of 16 MT px
  static constexpr int kNCQ = kNW / kNPG;          // channel groups of 32
  static constexpr int kCM = kTail[R].dt == DS ? 2 : 1;  // stored halves per logical channel (2: split fp16 pairs)
  static constexpr int kRowB = P * 2 * kCM;        // LDS bytes per pixel (bf16 / fp16 / split pairs)
  static constexpr int kWinCols = W + 2;
  static constexpr int kWinPix = (kRows + 2) * kWinCols;
  static constexpr int kBN2 = kWinPix * kRowB;     // s2 b2 f32 behind the window
  static constexpr int kLds = kBN2 + 2 * P * 4;
  static constexpr int kS3 = kPx * kRowB;          // s3 b3 f32 behind t2 (over the window)
  static constexpr int kKT = kCM * P / 32;         // k-steps per tap / per conv3 chunk (split: hi, lo per 32 ch)
  static constexpr int kChunk = 32 * kNCQ;         // conv3 output channels per chunk
  static constexpr int kNC = C / kChunk;           // conv3 chunks
  // stream blocks per conv3 chunk (+ DOWN: the downsample's K slice over x; + NEXT: the next conv1's)
  static constexpr int kBlk3 = 1 + DOWN + NEXT * NX;
  static constexpr int kSteps = 9 * kKT + kNC * kKT * kBlk3;
  static constexpr int kYC = kS3 + 2 * C * 4;      // NEXT: the y chunk [kPx][P] behind BN3
  static constexpr int kLdsN = NEXT && kYC + kPx * kRowB > kLds ? kYC + kPx * kRowB : kLds;
  // DOWN: the tile's block-input pixels (the downsample's B operand, P channels) behind everything
  // else, staged by LDS-DMA at the start beside the window
  static constexpr int kX0 = kLdsN;
  static constexpr int kLdsAll = DOWN ? kX0 + kPx * kRowB : kLdsN;
  static constexpr int kNB = kTail[R].nb;
  static constexpr int kD = kTail[R].kd < kKT ? kTail[R].kd : kKT;
  static constexpr int kKM = kKeyMask<kRowB>;
  static_assert(kNPG * kNCQ == kNW && kNPG >= 1 && kPx % (16 * kMT) == 0 && (16 * kMT) % W == 0,
                "every wave: 16 MT px (whole image rows) x 32 channels");
  // W = 24 (R152@384's layer3, round 5): m-tiles straddle image rows -- m-tile i = 3 m + c holds
  // tile pixels 48 m + 16 c .. (rows 2 m, 2 m + 1), three lane-address classes c
  static_assert(W % 16 == 0 || (W == 24 && kMT % 3 == 0 && kNPG == 1), "W a multiple of 16, or 24 in 3-m-tile periods");
  static_assert(kS3 + 2 * C * 4 <= kBN2, "t2 and BN3 fit over the window");
  static_assert(kLdsAll <= 160 * 1024, "LDS");
  static_assert(!NEXT || kChunk == P, "the next conv1 takes one y chunk per K slice of P channels");
  static_assert(kKT % kD == 0, "the ring slot of a k-step is static inside a block");
  static_assert(kCM == 1 || (kD % 2 == 0 && kNB == 2 && W % 16 == 0), "split pairs: even stream depth, two fragment sets");
  static_assert(static_cast<long long>(kNCQ) * kSteps * 2 * 1024 == stream_bytes(kTail[R]), "the host's stream size");
};

template <typename T, int R>
__global__ __launch_bounds__(kTail[R].nw * 64, kTail[R].wgs) void tail_stream_kernel(TailGeom g) {
  using O = Op<T>;
  // split fp16 (POSU_F16X3, round 6): every pixel row holds [hi 32 | lo 32] per 32 channels, i.e. the
  // kernel is the same GEMM over twice the K (kblock's hi / lo k-step pairs); the epilogues join
  // residual pairs and split their outputs
  constexpr bool SPL = O::SPLIT;
  using K = TailCfg<R>;
  static_assert(SPL == (kTail[R].dt == DS) && sizeof(T) == 2, "the row's dtype class");
  constexpr int W = K::W, P = K::P, C = K::C, NX = K::NX, CM = K::kCM, MT = K::kMT, NW = K::kNW;
  constexpr bool NEXT = K::NEXT, DOWN = K::DOWN;
  constexpr int kRows = K::kRows, kThreads = NW * 64;
  constexpr int ES = 2;
  __shared__ __attribute__((aligned(16))) char smem[K::kLdsAll];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int wu = __builtin_amdgcn_readfirstlane(wid);
  const int pg = wu / K::kNCQ, cq = wu - pg * K::kNCQ;
  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) char*)smem));
  const int H = g.H;
  const int tiles_per_img = H / kRows;
  const int n = blockIdx.x / tiles_per_img;
  const int y0 = (blockIdx.x - n * tiles_per_img) * kRows;
  float* bn2 = reinterpret_cast<float*>(smem + K::kBN2);
  for (int c = tid; c < P; c += kThreads) {
    bn2[c] = g.s2[c];
    bn2[P + c] = g.b2[c];
  }

  // ---- the t1 window: 1 KB wave-instructions (1024 / kRowB pixels each), instruction m by wave m & 7
  {
    constexpr int kPixPerInst = 1024 / K::kRowB, kInst = K::kWinPix / kPixPerInst;
    static_assert(K::kWinPix % kPixPerInst == 0, "whole instructions");
    constexpr int kChunks = K::kRowB / 16;
    const u32x4 t1s = make_srd(g.t1, g.N * H * W * P * CM * ES);
    const int sub = lane / kChunks, pc = lane % kChunks;
#pragma unroll
    for (int k = 0; k < (kInst + NW - 1) / NW; ++k) {
      const int m = wid + NW * k;
      if (m < kInst) {  // wave-uniform
        const int pix = kPixPerInst * m + sub;
        const int wr = pix / K::kWinCols, wc = pix - wr * K::kWinCols;
        const int yy = y0 + wr - 1, xx = wc - 1;
        const int lc = pc ^ (wkey<W>(wr, wc) & K::kKM);
        const bool ok = static_cast<unsigned>(yy) < static_cast<unsigned>(H) && static_cast<unsigned>(xx) < W;
        dma16(t1s, ok ? (((n * H + yy) * W + xx) * P * CM + 8 * lc) * ES : kOOB, lds0 + static_cast<unsigned>(m) * 1024u);
      }
    }
    if constexpr (DOWN) {
      // the block input's tile pixels (x: [N][H][W][P], the rows y0 .. y0 + kRows - 1 contiguous),
      // pixel p's chunks keyed by its column & 15 (the t2 image's layout)
      constexpr int kXInst = K::kPx / kPixPerInst;
      static_assert(K::kPx % kPixPerInst == 0, "whole instructions");
      const u32x4 xs = make_srd(g.x, g.N * H * W * P * CM * ES);
#pragma unroll
      for (int k = 0; k < (kXInst + NW - 1) / NW; ++k) {
        const int m = wid + NW * k;
        if (m < kXInst) {
          const int pix = kPixPerInst * m + sub;
          const int lc = pc ^ ((pix % W) & K::kKM);
          dma16(xs, ((n * H + y0) * W * P * CM + pix * P * CM + 8 * lc) * ES,
                lds0 + static_cast<unsigned>(K::kX0 + m * 1024));
        }
      }
    }
  }

  // ---- the weight stream of channel group cq; the window (LDS-DMA) and the first fragments
  WStream<K::kD, K::kSteps> ws(g.wst, cq, lane);
  ws.start(g, kThreads);

  f32x4 acc[MT][2];   // [m-tile i: tile pixels 16 MT pg + 16 i ..][n-tile j]
  f32x4 acc1[NX][MT][2];  // NEXT: the next conv1's accumulators over the whole chunk loop
  const int c32 = 32 * cq + cpair(q);   // this lane's 8 channels of the wave's 32
  constexpr bool kLateRes = NEXT;   // residual loads after a chunk's MFMAs
  // m-tile i's tile pixel (row-major in the tile) for this lane
  auto tpix = [&](int i) { return 16 * MT * pg + 16 * i + r16; };
  // a block over the tile's pixels in an image laid out like t2 (t2, x, the y chunk)
  auto tile_block = [&](f32x4 (&a)[MT][2], int blk, int base) {
    kblock<O, K::kKT, K::kNB>(a, ws, K::kKT * blk, RowsAddr<K::kRowB, W, W>(smem + base, tpix(0), r16, q));
  };

  // ---- conv2: 9 taps x kKT channel steps over the window
  zero(acc);
#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    const int dy = t / 3, dx = t - 3 * (t / 3);
    if constexpr (W % 16 != 0) {
      kblock<O, K::kKT, K::kNB>(acc, ws, K::kKT * t, Win24Addr<K::kRowB, K::kWinCols>(smem, dy, dx, r16, q));
    } else {
      // window pixel of m-tile i: tile row (16 MT pg + 16 i) / W + dy, column (16 i) % W + r16 + dx
      kblock<O, K::kKT, K::kNB>(acc, ws, K::kKT * t,
                                RowsAddr<K::kRowB, W, K::kWinCols>(smem, ((16 * MT / W) * pg + dy) * K::kWinCols + r16 + dx,
                                                                   wkey<W>(0, r16 + dx), q));
    }
  }
  const T* xg = reinterpret_cast<const T*>(g.x) + static_cast<size_t>(n * H + y0) * W * C * CM;
  T* yg = reinterpret_cast<T*>(g.y) + static_cast<size_t>(n * H + y0) * W * C * CM;
  // the tile's x / y (/ t1n) through buffer descriptors: a lane's 32-bit byte offset plus
  // compile-time per-m-tile / per-chunk steps, instead of a 64-bit address per m-tile (the
  // chained layer3 tail spilled such addresses: 34 VGPRs, round 4); stores keep soffset 0 (the
  // store-data hazard)
  const __amdgpu_buffer_rsrc_t xrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(xg), 0, K::kPx * C * CM * ES, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yg, 0, K::kPx * C * CM * ES, 0x00020000);
  // m-tile 0, chunk 0 (split: the hi half; the lo half 32 elements = 64 B further)
  const int lane_xy = (tpix(0) * C * CM + (SPL ? split_ch(c32) : c32)) * ES;
  auto xy_off = [&](int i, int nc) { return lane_xy + (16 * i * C + K::kChunk * nc) * CM * ES; };
  // conv3 chunk nc's residual in the epilogue's lane layout (rl: the split pairs' lo halves)
  auto res_load = [&](int nc, uint4 (&rv)[MT], uint4 (&rl)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(xrs, xy_off(i, nc), 0, 0);
      rv[i] = make_uint4(v[0], v[1], v[2], v[3]);
      if constexpr (SPL) {
        const auto l = __builtin_amdgcn_raw_buffer_load_b128(xrs, xy_off(i, nc) + 64, 0, 0);
        rl[i] = make_uint4(l[0], l[1], l[2], l[3]);
      }
    }
  };
  // 16-B store of the 8 values of this lane (split: the hi and the lo halves, 64 B apart)
  auto st8 = [&](__amdgpu_buffer_rsrc_t rs, int off, const float* v) {
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    if constexpr (SPL) {
      uint4 h, l;
      split8(v, h, l);
      __builtin_amdgcn_raw_buffer_store_b128(u4v{h.x, h.y, h.z, h.w}, rs, off, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(u4v{l.x, l.y, l.z, l.w}, rs, off + 64, 0, 0);
    } else {
      const uint4 o = O::store_vals(v);
      __builtin_amdgcn_raw_buffer_store_b128(u4v{o.x, o.y, o.z, o.w}, rs, off, 0, 0);
    }
  };
  // BN2 + ReLU -> t2 over the window (every wave is done reading it first), BN3 beside it
  lds_barrier();
  {
    float* b3l = reinterpret_cast<float*>(smem + K::kS3);
    for (int c = tid; c < C; c += kThreads) {
      b3l[c] = g.s3[c];
      b3l[C + c] = g.b3[c];
    }
    float sc[8], sh[8];
    ld8(bn2 + c32, sc);
    ld8(bn2 + P + c32, sh);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v[8];
      pair(acc, i, v);
      bn_relu(v, sc, sh, nullptr);
      lds_store8<O, K::kRowB>(smem, tpix(i), r16, c32 >> 3, v);
    }
  }
  lds_barrier();

  // ---- conv3: output chunk nc (kChunk channels; this wave's 32), kKT channel steps over t2
  const float* b3l = reinterpret_cast<const float*>(smem + K::kS3);
  auto chunk = [&](int nc, uint4 (&rv)[MT], uint4 (&rl)[MT]) {
    const int c0 = K::kChunk * nc + c32;
    zero(acc);
    tile_block(acc, 9 + K::kBlk3 * nc, 0);
    // DOWN: the downsample's K slice over the block input into the same accumulators
    if constexpr (DOWN) tile_block(acc, 9 + K::kBlk3 * nc + 1, K::kX0);
    // NEXT: the residual after the MFMAs (the next conv1's accumulators take its registers)
    if constexpr (kLateRes && !DOWN) res_load(nc, rv, rl);
    float sc[8], sh[8];
    ld8(b3l + c0, sc);
    ld8(b3l + C + c0, sh);
    if constexpr (NEXT) {
      if (nc > 0) lds_barrier();  // every wave is done reading the previous y chunk
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v[8], r[8];
      pair(acc, i, v);
      if constexpr (DOWN) {
        bn_relu(v, sc, sh, nullptr);   // no residual: the downsample is in the accumulators
      } else {
        if constexpr (SPL) join8(rv[i], rl[i], r);
        else O::load_vals(rv[i], r);
        bn_relu(v, sc, sh, r);
      }
      st8(yrs, xy_off(i, nc), v);
      // NEXT: the chunk's y, laid out like t2 ([pixel][P] rows, column-keyed swizzle)
      if constexpr (NEXT) lds_store8<O, K::kRowB>(smem + K::kYC, tpix(i), r16, c32 >> 3, v);
    }
    if constexpr (NEXT) {
      // the next block's conv1 over this K slice (y channels kChunk nc ..): same k order as a
      // conv launch over y, so t1n is bit-identical to it
      lds_barrier();
#pragma unroll
      for (int h = 0; h < NX; ++h) tile_block(acc1[h], 9 + K::kBlk3 * nc + 1 + DOWN + h, K::kYC);
    }
  };
  // unrolled: hipcc's wait counts at a loop head merge both paths and made every chunk's first
  // weight wait also wait for the previous chunk's y stores (layer2 tail 90.7 -> 86.7 us)
  if constexpr (NEXT) {
#pragma unroll
    for (int h = 0; h < NX; ++h) zero(acc1[h]);
  }
#pragma unroll
  for (int nc = 0; nc < K::kNC; ++nc) {
    // the chunk's residual, kKT k-steps ahead of its epilogue (the weight fragments consumed
    // meanwhile were loaded before it: the in-order vmcnt does not hold them back)
    uint4 rv[MT], rl[MT];
    if constexpr (!kLateRes && !DOWN) res_load(nc, rv, rl);
    chunk(nc, rv, rl);
  }
  if constexpr (NEXT) {
    // t1n = relu(conv1n * s1n + b1n) [.., NX P], this lane's 8 channels (of each half) of each m-tile's pixel
    constexpr int PN = NX * P;
    T* tg = reinterpret_cast<T*>(g.t1n) + static_cast<size_t>(n * H + y0) * W * PN * CM;
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(tg, 0, K::kPx * PN * CM * ES, 0x00020000);
#pragma unroll
    for (int h = 0; h < NX; ++h) {
      const int c0 = h * P + c32;
      float sc[8], sh[8];
      ld8(g.s1n + c0, sc);
      ld8(g.b1n + c0, sh);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        float v[8];
        pair(acc1[h], i, v);
        bn_relu(v, sc, sh, nullptr);
        st8(trs, (tpix(i) * PN * CM + (SPL ? split_ch(c0) : c0)) * ES, v);
      }
    }
  }
}

template <int R>
void launch_row(int dtype, const TailGeom& g, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(g.N * (g.H / kTail[R].rows))), block(kTail[R].nw * 64);
  if constexpr (kTail[R].dt == DS) hipLaunchKernelGGL((tail_stream_kernel<f16s_t, R>), grid, block, 0, s, g);
  else if (dtype == POSU_BF16) hipLaunchKernelGGL((tail_stream_kernel<uint16_t, R>), grid, block, 0, s, g);
  else hipLaunchKernelGGL((tail_stream_kernel<f16_t, R>), grid, block, 0, s, g);
}
template <size_t... R>
void launch_tail(int row, int dtype, const TailGeom& g, hipStream_t s, std::index_sequence<R...>) {
  ((row == static_cast<int>(R) ? launch_row<static_cast<int>(R)>(dtype, g, s) : void()), ...);
}

}  // namespace
}  // namespace posu

using namespace posu;

namespace {
int tail_stream_impl(const char* name, int dtype, const void* t1, const void* x, int N, int H, int W, int C, int P,
                     const void* wstream, long long wstream_bytes, const float* s2, const float* b2,
                     const float* s3, const float* b3, void* y, const float* s1n, const float* b1n, void* t1n,
                     void* stream, bool down = false, int nx = 1) {
  const std::string what = name;
  const bool next = t1n != nullptr;
  const bool spl = dtype == POSU_F16X3;
  POSU_REQUIRE(dtype == POSU_BF16 || dtype == POSU_F16 || spl, what + ": dtype must be BF16, F16 or F16X3");
  POSU_REQUIRE(s3, what + ": null pointer");
  TailGeom g;
  if (int e = tail_operands(g, what, t1, x, N, H, wstream, wstream_bytes, s2, b2, s3, b3, y, s1n, b1n, t1n)) return e;
  // one walk over the table: the launch's row, and what the table has for its shape (for the refusals)
  const unsigned cls = spl ? DS : D2;
  const bool small = N > 0 && H % 4 == 0 && static_cast<long long>(N) * (H / 8) < kSmallGridWGs;
  int row = -1;
  bool shape = false, shape_cls = false, has_down = false, has_nx2 = false;
  for (int i = 0; i < kNTail; ++i) {
    const TailRow& r = kTail[i];
    if (r.W != W || r.P != P || r.C != C) continue;
    shape = true;
    if (!(r.dt & cls)) continue;
    shape_cls = true;
    has_down |= r.down;
    has_nx2 |= r.nx == 2;
    if (r.next == next && r.down == down && r.nx == nx && (r.grid == kAnyGrid || (r.grid == kSmallGrid) == small)) row = i;
  }
  POSU_REQUIRE(shape_cls || (spl && shape),
               what + ": built for layer2 (W = 32 or 48, C = 512, planes = 128) and layer3 (W = 16 or 24, C = 1024, "
                      "planes = 256) of PoseResNet at 256x256 / 384x384, layer1 at 384x384 (W = 96, C = 256, planes "
                      "64; BF16 / F16) and (split fp16) layer1 at 256x256 (W = 64)");
  POSU_REQUIRE(shape_cls, what + ": the split dtype runs the 256x256 tails (W = 64, 32, 16)");
  POSU_REQUIRE(!down || has_down,
               what + ": built for layer1's first Bottleneck (x 64 -> y 256 channels, planes 64) at W = 64 in split "
                      "fp16 and at W = 96 in BF16 / F16");
  POSU_REQUIRE(nx == 1 || (nx == 2 && next && !down && has_nx2),
               what + ": a next conv1 of 2 P outputs is chained by the 256x256 identity tails only (layer1: split)");
  POSU_REQUIRE(row >= 0, what + ": no variant for this launch");
  const int cm = spl ? 2 : 1;   // stored halves per logical channel
  if (int e = tail_sizes(g, what, kTail[row].rows, static_cast<long long>(N) * H * W * C * 2 * cm, wstream_bytes,
                         stream_bytes(kTail[row])))
    return e;
  launch_tail(row, dtype, g, as_stream(stream), std::make_index_sequence<kNTail>{});
  return check_launch(name);
}
}  // namespace

extern "C" int posu_bottleneck_tail_stream_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C,
                                               int P, const void* wstream, long long wstream_bytes,
                                               const float* s2, const float* b2, const float* s3, const float* b3,
                                               void* y, void* stream) {
  return tail_stream_impl("posu_bottleneck_tail_stream_fwd", dtype, t1, x, N, H, W, C, P, wstream, wstream_bytes, s2,
                          b2, s3, b3, y, nullptr, nullptr, nullptr, stream);
}

// Chained identity Bottlenecks: the tail above, and the NEXT identity block's conv1 (+ BN1 +
// ReLU) over this block's output y while its chunks are produced -- t1n, which the next
// block's tail takes instead of a conv1 launch over y.  wstream = packing.pack_tail_stream
// (conv2, conv3, next conv1).
extern "C" int posu_bottleneck_tail_stream_next_fwd(int dtype, const void* t1, const void* x, int N, int H, int W,
                                                    int C, int P, const void* wstream, long long wstream_bytes,
                                                    const float* s2, const float* b2, const float* s3,
                                                    const float* b3, void* y, const float* s1n, const float* b1n,
                                                    void* t1n, void* stream) {
  if (!t1n) {
    set_error("posu_bottleneck_tail_stream_next_fwd: null pointer (t1n)");
    return POSU_ERR_ARG;
  }
  return tail_stream_impl("posu_bottleneck_tail_stream_next_fwd", dtype, t1, x, N, H, W, C, P, wstream,
                          wstream_bytes, s2, b2, s3, b3, y, s1n, b1n, t1n, stream);
}

// Layer1's first Bottleneck (split fp16, round 6): conv2 + [conv3 | downsample] dual GEMM + ReLU in one
// launch (the downsample over the block input x [N, H, 64, P] staged in LDS), optionally chained with
// the next block's conv1 (t1n != nullptr).  s3 / b3: the dual GEMM's scale / shift (b3 + bd);
// wstream = packing.pack_down_tail_stream(conv2 pack, dual pack[, next conv1 pack]).
extern "C" int posu_bottleneck_down_tail_stream_fwd(int dtype, const void* t1, const void* x, int N, int H, int W,
                                                    int C, int P, const void* wstream, long long wstream_bytes,
                                                    const float* s2, const float* b2, const float* s3,
                                                    const float* b3, void* y, const float* s1n, const float* b1n,
                                                    void* t1n, void* stream) {
  return tail_stream_impl("posu_bottleneck_down_tail_stream_fwd", dtype, t1, x, N, H, W, C, P, wstream, wstream_bytes,
                          s2, b2, s3, b3, y, s1n, b1n, t1n, stream, true);
}

// The last identity block of a layer chained with the NEXT layer's first conv1 (1x1, C -> Pn = 2 P at this
// map size; the strided block's conv2 / dual GEMM follow as their own launches), split fp16 only (round 6):
// t1n [N, H, W, Pn] (logical), s1n / b1n [Pn]; wstream = packing.pack_tail_stream(conv2, conv3, next conv1
// pack [Pn][C']).  Pn = P is posu_bottleneck_tail_stream_next_fwd.
extern "C" int posu_bottleneck_tail_stream_chain_fwd(int dtype, const void* t1, const void* x, int N, int H, int W,
                                                     int C, int P, int Pn, const void* wstream,
                                                     long long wstream_bytes, const float* s2, const float* b2,
                                                     const float* s3, const float* b3, void* y, const float* s1n,
                                                     const float* b1n, void* t1n, void* stream) {
  if (!t1n || P <= 0 || (Pn != P && Pn != 2 * P)) {
    set_error("posu_bottleneck_tail_stream_chain_fwd: t1n must be given and Pn must be P or 2 P");
    return POSU_ERR_ARG;
  }
  return tail_stream_impl("posu_bottleneck_tail_stream_chain_fwd", dtype, t1, x, N, H, W, C, P, wstream, wstream_bytes,
                          s2, b2, s3, b3, y, s1n, b1n, t1n, stream, false, Pn / P);
}
