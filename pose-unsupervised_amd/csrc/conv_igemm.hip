// Implicit-GEMM convolution on CDNA4 MFMA, NHWC activations.
//
// GEMM view of one launch:  rows m = output pixels (n, oy, ox) of the launch grid,
//                           cols   = output channels,
//                           k      = (kh, kw, ci) taps of the input window.
// A[m][k] is gathered on the fly from the NHWC input (16-byte channel chunks,
// out-of-window taps read as zeros through a buffer descriptor), B[k][co] is the
// packed weight [CoutPad][Kpad] (K contiguous, zero padded).
//
// Block tile BM x BN (BM in {64, 128}, BN in {64, 128}), K-tile of 128 bytes per row
// (64 bf16 / 32 f32), 256 threads = 4 waves in a 2x2 grid, each wave owning a
// (BM/2) x (BN/2) accumulator tile made of 16x16 MFMA tiles:
//   bf16: v_mfma_f32_16x16x32_bf16 (one 16-B chunk per lane = one MFMA k-step)
//   f32 : v_mfma_f32_16x16x4_f32   (one 16-B chunk per lane = four MFMA k-steps;
//         the k order inside a chunk is permuted identically for A and B, which
//         leaves the sum unchanged)
// Pipeline: global->register prefetch of K-tile t+1 while the MFMAs of tile t run
// out of LDS buffer t&1; the registers are written to the other LDS buffer after
// the MFMAs; one barrier per K-tile.  LDS rows are 128 B with the 16-B chunk index
// XOR-swizzled by (row>>1)&7, which makes the 16-lane ds_read_b128 groups of the
// fragment reads conflict-free.
//
// DUAL variant (Bottleneck tail with a downsample branch, pose_resnet.py:90-99,
// 136-141): two 1x1 sources share one accumulator,
//   y = act( [W3*s3 | Wd*sd] . [conv2_out(m) ; block_in(n, oy*s, ox*s)] + (b3 + bd) ),
// so the downsample output is never written to / re-read from HBM.
//
// Epilogue: residual chunks are prefetched into registers first; the accumulators
// (+BN scale/shift) are staged through LDS as an f32 tile, then written as 16-byte
// NHWC chunks with residual add + ReLU, or as NCHW f32 heatmaps (+bias) for the
// final 1x1 layer (pose_resnet.py:126-132).
//
// ConvTranspose2d(4, s2, p1) runs as 4 sub-pixel 2x2 stride-1 convolutions, one per
// output parity class (py, px) = blockIdx.z: output (2*qy+py, 2*qx+px) reads inputs
// qy + py - 1 + ty, qx + px - 1 + tx with the deconv tap (3-py-2ty, 3-px-2tx);
// the Python layer packs those taps per class.
#include <string>

#include "conv_igemm_kernels.h"

namespace posu {
namespace {

int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

template <typename T, int BM, int BN, int NW, int WGM, bool DUAL>
void launch_persist(const ConvGeom& g, int ntile, hipStream_t s) {
  // four-wave tiles keep two slots (several blocks per CU hide each other's latencies);
  // eight-wave tiles take a third slot where it fits
  constexpr int S = (NW == 8 && ring_bytes<BM, BN, 3>() <= 160 * 1024) ? 3 : 2;
  static const int occ = [] {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, conv_persist_kernel<T, BM, BN, NW, WGM, S, DUAL>, NW * 64,
                                                     0) != hipSuccess || b < 1)
      b = 1;
    return b;
  }();
  int grid = std::min(ntile, cu_count() * occ);
  grid = std::max(8, grid & ~7);  // whole XCD rounds (blockIdx & 7 = XCD slice)
  hipLaunchKernelGGL((conv_persist_kernel<T, BM, BN, NW, WGM, S, DUAL>), dim3(grid), dim3(NW * 64), 0, s, g);
}

// ---- Tile configurations (the `tile` argument of the conv entry points).  kTiles is the whole
// story: tile id -> kernel instance = shape (tile, waves, wave grid) + main loop, per dtype class.
// The first row with the id and the launch's dtype class is the id's row for that class; an id
// without one is refused ("tile must be").  Where a row does not hold for a launch -- the tile's BN
// does not divide CoutPad, or its loop's own condition below fails -- the id in its last column
// runs instead (-1: the heuristic).
enum Shape {
  k256x64, k128x64, k64x64, k128x128, k64x128,  // four waves
  k256x256, k256x128,                            // eight waves
  // (round 4) 128x128 with eight waves, as 2x4 waves of 64x32 / 4x2 waves of 32x64 (M = 8192-pixel
  // layers: 256 tiles of 128x128 give every CU one block, and eight waves two per SIMD)
  k128x128w24, k128x128w42,
};
struct ShapeDim {
  int bm, bn;
};
constexpr ShapeDim kDim[] = {{256, 64},  {128, 64},  {64, 64},   {128, 128}, {64, 128},
                             {256, 256}, {256, 128}, {128, 128}, {128, 128}};
enum Loop {
  kRing1,    // single-slot LDS ring (four-wave shapes; short-K layers: more blocks per CU)
  kRing2,    // two-slot ring
  kRing3,    // three-slot ring
  kStagger,  // two slots, waves 4-7 half a K-tile behind (eight-wave shapes)
  kKGroups,  // two K groups of four waves (the only loop with its own K order); mode 0, no head
  kPersist,  // the persistent K-tile stream (conv_persist_kernel, its slot count fixed per shape):
             // bf16 / f16, mode 0, outputs addressable by a 32-bit buffer offset
  kAuto,     // accepted, runs the heuristic
};
enum : unsigned { D2 = 1, DS = 2, DF = 4, ALL = 7 };  // dtype class: bf16 / f16, split fp16, f32
struct TileRow {
  int id;
  unsigned dt;
  Shape shape;
  Loop loop;
  int fb;
};
constexpr TileRow kTiles[] = {
    // cfg + 8 * variant: cfg 0-6 = the seven plain shapes, variant 0 / 1 / 2 = ring of 2 / 1 / 3 slots
    {0, ALL, k256x64, kRing2, -1},
    {1, ALL, k128x64, kRing2, -1},
    {2, ALL, k64x64, kRing2, -1},
    {3, ALL, k128x128, kRing2, -1},
    {4, ALL, k64x128, kRing2, -1},
    {5, ALL, k256x256, kRing2, -1},
    {6, ALL, k256x128, kRing2, -1},
    {8, ALL, k256x64, kRing1, -1},
    {9, ALL, k128x64, kRing1, -1},
    {10, ALL, k64x64, kRing1, -1},
    {11, ALL, k128x128, kRing1, -1},
    {12, ALL, k64x128, kRing1, -1},
    {16, ALL, k256x64, kRing3, -1},
    {17, ALL, k128x64, kRing3, -1},
    {18, ALL, k64x64, kRing3, -1},
    {19, ALL, k128x128, kRing3, -1},
    {20, ALL, k64x128, kRing3, -1},
    {22, ALL, k256x128, kRing3, -1},
    // + 32: the persistent stream of the same shape; where it does not hold (other dtypes among
    // the reasons) the id without the bit.  (No persistent 256x64 instance: dynamic indexing of its
    // store registers put 960 B per lane in scratch; 32 / 40 / 48 run the plain 256x64 tile.)
    {32, ALL, k256x64, kRing2, -1},
    {33, ALL, k128x64, kPersist, 1},
    {34, ALL, k64x64, kPersist, 2},
    {35, ALL, k128x128, kPersist, 3},
    {36, ALL, k64x128, kPersist, 4},
    {37, ALL, k256x256, kPersist, 5},
    {38, ALL, k256x128, kPersist, 6},
    {40, ALL, k256x64, kRing1, -1},
    {41, ALL, k128x64, kPersist, 9},
    {42, ALL, k64x64, kPersist, 10},
    {43, ALL, k128x128, kPersist, 11},
    {44, ALL, k64x128, kPersist, 12},
    {48, ALL, k256x64, kRing3, -1},
    {49, ALL, k128x64, kPersist, 17},
    {50, ALL, k64x64, kPersist, 18},
    {51, ALL, k128x128, kPersist, 19},
    {52, ALL, k64x128, kPersist, 20},
    {54, ALL, k256x128, kPersist, 22},
    // the eight-wave 128x128 tiles: staggered in bf16 / f16, unstaggered in split fp16 (whose
    // staggered twins are 47 / 55, round 6)
    {7, D2, k128x128w24, kStagger, -1},
    {7, DS, k128x128w24, kRing2, -1},
    {7, DF, k128x128w24, kAuto, -1},
    {15, D2, k128x128w42, kStagger, -1},
    {15, DS, k128x128w42, kRing2, -1},
    {15, DF, k128x128w42, kAuto, -1},
    {47, DS, k128x128w24, kStagger, -1},
    {55, DS, k128x128w42, kStagger, -1},
    // 256x256 / 256x128 staggered (also what the heuristic runs for those shapes in bf16 / f16)
    // (split fp16: 31 only -- its staggered 256x256 instance spills 56 VGPRs)
    {23, D2, k256x256, kStagger, -1},
    {23, DS | DF, k256x256, kAuto, -1},
    {31, D2 | DS, k256x128, kStagger, -1},
    {31, DF, k256x128, kAuto, -1},
    // (round 5) 128x128 as two K groups
    {39, D2 | DS, k128x128w24, kKGroups, -1},
    {39, DF, k128x128w24, kAuto, -1},
};

template <typename T>
constexpr unsigned dclass() {
  return Op<T>::SPLIT ? DS : sizeof(T) == 2 ? D2 : DF;
}
unsigned dclass_of(int dtype) { return dtype == POSU_F16X3 ? DS : (dtype == POSU_BF16 || dtype == POSU_F16) ? D2 : DF; }

const TileRow* tile_row(int id, unsigned cls) {
  for (const TileRow& r : kTiles)
    if (r.id == id && (r.dt & cls)) return &r;
  return nullptr;
}
bool tile_ok(int dtype, int tile) { return tile == -1 || tile_row(tile, dclass_of(dtype)) != nullptr; }
// the entry points' refusal: "<what>: tile must be -1 (auto) or one of <the dtype's ids>"
std::string tile_error(const char* what, int dtype) {
  std::string ids;
  for (int id = 0; id < 64; ++id)
    if (tile_row(id, dclass_of(dtype))) ids += (ids.empty() ? "" : ", ") + std::to_string(id);
  return std::string(what) + ": tile must be -1 (auto) or one of " + ids;
}

bool row_holds(const TileRow& r, unsigned cls, const ConvGeom& g) {
  if (r.loop == kAuto || g.CoutPad % kDim[r.shape].bn != 0) return false;
  if (r.loop == kKGroups) return g.mode == 0 && !g.hm;
  if (r.loop == kPersist)
    return cls == D2 && g.mode == 0 && static_cast<long long>(g.N) * g.out_H * g.out_W * g.Cout * 2 < (1LL << 31) - 256;
  return true;
}

struct Inst {
  Shape shape;
  Loop loop;
};
Inst resolve_tile(int tile, unsigned cls, const ConvGeom& g, int nclass) {
  for (int id = tile; id >= 0;) {
    const TileRow* r = tile_row(id, cls);
    if (!r) break;
    if (row_holds(*r, cls, g)) return {r->shape, r->loop};
    id = r->fb;
  }
  // heuristic: 64-channel layers take 256 x 64 tiles (four waves stacked along M, 64 x 64
  // each); wider layers 256 x 256 with eight 128 x 64 waves when the grid still gives
  // every CU a block, else 128 x 128; grids that would not give every CU two blocks drop
  // to 64-row tiles.
  auto blocks = [&](int bm, int bn) {
    return static_cast<long long>((g.M + bm - 1) / bm) * (g.CoutPad / bn) * nclass;
  };
  if (g.CoutPad % 128 != 0) return {blocks(256, 64) >= 1024 ? k256x64 : (blocks(128, 64) >= 512 ? k128x64 : k64x64), kRing2};
  // untuned eight-wave launches take the staggered loop (bit-exact with the plain one)
  if (g.CoutPad % 256 == 0 && blocks(256, 256) >= 256) return {k256x256, cls == D2 && tile == -1 ? kStagger : kRing2};
  // 128-channel layers: 256 x 128 measured slower than 128 x 128 (layer2 c1/c2, R50@256)
  return {blocks(128, 128) >= 512 ? k128x128 : k64x128, kRing2};
}

template <typename T, int BM, int BN, int NW, int WGM, int S, bool DUAL, bool SG = false, bool KS = false>
bool launch_tile(const ConvGeom& g, int blocks, hipStream_t s) {
  hipLaunchKernelGGL((conv_igemm_kernel<T, BM, BN, NW, WGM, S, DUAL, SG, false, KS>), dim3(blocks), dim3(NW * 64), 0,
                     s, g);
  return true;
}

// the instances of one shape: which loops it has in dtype T (false: none for `loop`)
template <typename T, int BM, int BN, int NW, int WGM, bool DUAL>
bool launch_shape(Loop loop, const ConvGeom& g, int blocks, hipStream_t s) {
  constexpr unsigned D = dclass<T>();
  constexpr bool W8 = NW == 8 && BM == 128;  // the eight-wave 128x128 tile
  switch (loop) {
    case kRing1:
      if constexpr (NW == 4) return launch_tile<T, BM, BN, NW, WGM, 1, DUAL>(g, blocks, s);
      break;
    case kRing2:
      if constexpr (!W8 || D == DS) return launch_tile<T, BM, BN, NW, WGM, 2, DUAL>(g, blocks, s);
      break;
    case kRing3:
      if constexpr (!W8 && ring_bytes<BM, BN, 3>() <= 160 * 1024)
        return launch_tile<T, BM, BN, NW, WGM, 3, DUAL>(g, blocks, s);
      break;
    case kStagger:
      // the split dtype staggers too (round 6), but not on 256x256
      if constexpr (NW == 8 && (D == D2 || (D == DS && !(BM == 256 && BN == 256))))
        return launch_tile<T, BM, BN, NW, WGM, 2, DUAL, true>(g, blocks, s);
      break;
    case kKGroups:
      if constexpr (W8 && WGM == 2 && D != DF) return launch_tile<T, BM, BN, NW, WGM, 2, DUAL, false, true>(g, blocks, s);
      break;
    case kPersist:
      if constexpr (D == D2 && !W8 && !(BM == 256 && BN == 64)) {
        launch_persist<T, BM, BN, NW, WGM, DUAL>(g, blocks, s);
        return true;
      }
      break;
    default: break;
  }
  return false;
}

template <typename T, bool DUAL>
bool launch_inst(Inst in, const ConvGeom& g, int blocks, hipStream_t s) {
  switch (in.shape) {
    case k256x64: return launch_shape<T, 256, 64, 4, 4, DUAL>(in.loop, g, blocks, s);
    case k128x64: return launch_shape<T, 128, 64, 4, 2, DUAL>(in.loop, g, blocks, s);
    case k64x64: return launch_shape<T, 64, 64, 4, 2, DUAL>(in.loop, g, blocks, s);
    case k128x128: return launch_shape<T, 128, 128, 4, 2, DUAL>(in.loop, g, blocks, s);
    case k64x128: return launch_shape<T, 64, 128, 4, 2, DUAL>(in.loop, g, blocks, s);
    case k256x256: return launch_shape<T, 256, 256, 8, 2, DUAL>(in.loop, g, blocks, s);
    case k256x128: return launch_shape<T, 256, 128, 8, 4, DUAL>(in.loop, g, blocks, s);
    case k128x128w24: return launch_shape<T, 128, 128, 8, 2, DUAL>(in.loop, g, blocks, s);
    case k128x128w42: return launch_shape<T, 128, 128, 8, 4, DUAL>(in.loop, g, blocks, s);
  }
  return false;
}

#ifndef POSU_SPLIT_SG_HEAD
#define POSU_SPLIT_SG_HEAD 0   // (the staggered split 256x256 head instance spills 23 VGPRs)
#endif
template <typename T, bool DUAL>
int launch(ConvGeom g, int nclass, hipStream_t s, const char* what, int tile) {
  constexpr bool SPL = Op<T>::SPLIT;
  {
    const long long wbytes = static_cast<long long>(g.CoutPad) * g.Kpad * static_cast<long long>(sizeof(T)) * nclass;
    g.warm = warm_wgs(wbytes);
    g.wseg = wbytes / 64;
  }
  if constexpr (sizeof(T) == 2 && !DUAL) {  // fused head on the eight-wave 256x256 tile, direct epilogue
    if (g.hm && g.CoutPad == 256) {
      g.ntiles = 1;
      g.mtiles = (g.M + 255) / 256;
      if constexpr (SPL) {
        // (round 6: the staggered loop in split fp16 too, POSU_SPLIT_SG_HEAD; bit-identical either way)
        hipLaunchKernelGGL((conv_igemm_kernel<T, 256, 256, 8, 2, 2, DUAL, POSU_SPLIT_SG_HEAD != 0, true>),
                           dim3(g.mtiles * nclass), dim3(512), 0, s, g);
      } else {
        // staggered two-slot loop (waves 4-7 half a K-tile behind; bit-exact with tile 5)
        hipLaunchKernelGGL((conv_igemm_kernel<T, 256, 256, 8, 2, 2, DUAL, true, true>), dim3(g.mtiles * nclass),
                           dim3(512), 0, s, g);
      }
      return check_launch(what);
    }
  }
  if (g.hm) {  // fused head (f32): one 64x256 block owns all 256 output channels, head from LDS
    g.ntiles = 1;
    g.mtiles = (g.M + 63) / 64;
    hipLaunchKernelGGL((conv_igemm_kernel<T, 64, 256, 4, 1, 2, DUAL>), dim3(g.mtiles * nclass), dim3(256), 0, s, g);
    return check_launch(what);
  }
  const Inst in = resolve_tile(tile, dclass<T>(), g, nclass);
  g.ntiles = g.CoutPad / kDim[in.shape].bn;
  g.mtiles = (g.M + kDim[in.shape].bm - 1) / kDim[in.shape].bm;
  if (!launch_inst<T, DUAL>(in, g, g.mtiles * g.ntiles * nclass, s)) {
    set_error(std::string(what) + ": the tile table names a kernel instance that does not exist");
    return POSU_ERR_ARG;
  }
  return check_launch(what);
}

template <bool DUAL>
int dispatch(int dtype, ConvGeom& g, int nclass, void* stream, const char* what, int tile = -1) {
  hipStream_t s = as_stream(stream);
  if (dtype == POSU_BF16) return launch<uint16_t, DUAL>(g, nclass, s, what, tile);
  if (dtype == POSU_F32) return launch<float, DUAL>(g, nclass, s, what, tile);
  if (dtype == POSU_F16) return launch<f16_t, DUAL>(g, nclass, s, what, tile);
  if (dtype == POSU_F16X3) return launch<f16s_t, DUAL>(g, nclass, s, what, tile);
  set_error(std::string(what) + ": unsupported dtype");
  return POSU_ERR_ARG;
}

// the direct epilogue reads the per-channel BN parameters as 16-B vectors
bool params_aligned(const float* scale, const float* shift) {
  return (reinterpret_cast<size_t>(scale) & 15) == 0 && (reinterpret_cast<size_t>(shift) & 15) == 0;
}

int bk_of(int dtype) { return dtype == POSU_F32 ? 32 : 64; }
int esz_of(int dtype) { return dtype == POSU_F32 ? 4 : 2; }
// stored elements per logical channel (the split dtype keeps a (hi, lo) pair)
int cm_of(int dtype) { return dtype == POSU_F16X3 ? 2 : 1; }

int common_checks(int dtype, const void* x, const void* w, const void* y, int N, int H, int W, int C,
                  int Cout, const char* what) {
  POSU_REQUIRE(dtype == POSU_BF16 || dtype == POSU_F32 || dtype == POSU_F16 || dtype == POSU_F16X3,
               std::string(what) + ": dtype must be F32, BF16, F16 or F16X3");
  POSU_REQUIRE(x && w && y, std::string(what) + ": null pointer");
  POSU_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0, std::string(what) + ": empty shape");
  POSU_REQUIRE(C >= 8 && ilog2(C) >= 0, std::string(what) + ": C must be a power of two >= 8");
  POSU_REQUIRE(dtype != POSU_F16X3 || (C % 32 == 0 && Cout % 32 == 0),
               std::string(what) + ": split fp16 needs C and Cout multiples of 32");
  POSU_REQUIRE(static_cast<long long>(N) * H * W * C * cm_of(dtype) * esz_of(dtype) < (1LL << 31) - 256,
               std::string(what) + ": input exceeds the 2 GiB buffer-descriptor range");
  return POSU_OK;
}

ConvGeom base_geom(const void* x, int N, int H, int W, int C, const void* w, int Cout, int dtype) {
  ConvGeom g{};
  g.x = x;
  g.w = w;
  g.N = N;
  g.H = H;
  g.W = W;
  g.C = C * cm_of(dtype);  // stored channels (the GEMM's K per tap)
  g.logC = ilog2(g.C);
  g.Cout = Cout;
  g.CoutPad = round_up(Cout, 64);
  g.stride = 1;
  g.KH = g.KW = 1;
  return g;
}

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" int posu_conv_bk(int dtype) { return bk_of(dtype); }

extern "C" int posu_conv2d_fwd(int dtype, const void* x, int N, int H, int W, int C, const void* w, int Cout,
                               int KH, int KW, int stride, int pad, const float* scale, const float* shift,
                               const void* residual, int relu, void* y, int Ho, int Wo, int tile, void* stream) {
  if (int st = common_checks(dtype, x, w, y, N, H, W, C, Cout, "posu_conv2d_fwd")) return st;
  POSU_REQUIRE(tile_ok(dtype, tile), tile_error("posu_conv2d_fwd", dtype));
  const int E = 16 / esz_of(dtype);
  POSU_REQUIRE(Cout % E == 0, "posu_conv2d_fwd: Cout must be a multiple of 16 bytes");
  POSU_REQUIRE(KH > 0 && KW > 0 && stride > 0 && pad >= 0, "posu_conv2d_fwd: bad window");
  POSU_REQUIRE(Ho > 0 && Wo > 0 && Ho <= (H + 2 * pad - KH) / stride + 1 && Wo <= (W + 2 * pad - KW) / stride + 1,
               "posu_conv2d_fwd: Ho/Wo larger than the window allows");
  POSU_REQUIRE(static_cast<long long>(N) * Ho * Wo * Cout * cm_of(dtype) < (1LL << 31),
               "posu_conv2d_fwd: output too large");
  POSU_REQUIRE(params_aligned(scale, shift), "posu_conv2d_fwd: scale / shift must be 16-byte aligned");
  ConvGeom g = base_geom(x, N, H, W, C, w, Cout, dtype);
  g.scale = scale;
  g.shift = shift;
  g.res = residual;
  g.y = y;
  g.Ho = Ho;
  g.Wo = Wo;
  g.M = N * Ho * Wo;
  g.K = KH * KW * g.C;
  g.Kpad = round_up(g.K, bk_of(dtype));
  g.KH = KH;
  g.KW = KW;
  g.stride = stride;
  g.pad_h = pad;
  g.pad_w = pad;
  g.relu = relu;
  g.out_H = Ho;
  g.out_W = Wo;
  return dispatch<false>(dtype, g, 1, stream, "posu_conv2d_fwd", tile);
}

extern "C" int posu_conv1x1_dual_fwd(int dtype, const void* x, int N, int H, int W, int C, const void* x2, int H2,
                                     int W2, int C2, int stride2, const void* w, int Cout, const float* scale,
                                     const float* shift, int relu, void* y, int tile, void* stream) {
  if (int st = common_checks(dtype, x, w, y, N, H, W, C, Cout, "posu_conv1x1_dual_fwd")) return st;
  POSU_REQUIRE(tile_ok(dtype, tile), tile_error("posu_conv1x1_dual_fwd", dtype));
  if (int st = common_checks(dtype, x2, w, y, N, H2, W2, C2, Cout, "posu_conv1x1_dual_fwd")) return st;
  const int BK = bk_of(dtype);
  // (the NHWC epilogues store whole 16-byte channel chunks, as in posu_conv2d_fwd)
  POSU_REQUIRE(Cout % (16 / esz_of(dtype)) == 0, "posu_conv1x1_dual_fwd: Cout must be a multiple of 16 bytes");
  POSU_REQUIRE(C % BK == 0 && C2 % BK == 0, "posu_conv1x1_dual_fwd: C and C2 must be multiples of the K-tile");
  POSU_REQUIRE(stride2 > 0 && (H - 1) * stride2 < H2 && (W - 1) * stride2 < W2,
               "posu_conv1x1_dual_fwd: source-2 grid too small for the output grid");
  POSU_REQUIRE(static_cast<long long>(N) * H * W * Cout * cm_of(dtype) < (1LL << 31),
               "posu_conv1x1_dual_fwd: output too large");
  POSU_REQUIRE(params_aligned(scale, shift), "posu_conv1x1_dual_fwd: scale / shift must be 16-byte aligned");
  ConvGeom g = base_geom(x, N, H, W, C, w, Cout, dtype);
  g.x2 = x2;
  g.H2 = H2;
  g.W2 = W2;
  g.C2 = C2 * cm_of(dtype);
  g.stride2 = stride2;
  g.K1 = g.C;
  g.scale = scale;
  g.shift = shift;
  g.y = y;
  g.Ho = H;
  g.Wo = W;
  g.M = N * H * W;
  g.K = g.C + g.C2;
  g.Kpad = g.C + g.C2;
  g.relu = relu;
  g.out_H = H;
  g.out_W = W;
  return dispatch<true>(dtype, g, 1, stream, "posu_conv1x1_dual_fwd", tile);
}

extern "C" int posu_deconv4x4s2_fwd(int dtype, const void* x, int N, int H, int W, int C, const void* w,
                                    int Cout, const float* scale, const float* shift, int relu, void* y, int tile,
                                    void* stream) {
  if (int st = common_checks(dtype, x, w, y, N, H, W, C, Cout, "posu_deconv4x4s2_fwd")) return st;
  POSU_REQUIRE(tile_ok(dtype, tile), tile_error("posu_deconv4x4s2_fwd", dtype));
  const int E = 16 / esz_of(dtype);
  POSU_REQUIRE(Cout % E == 0, "posu_deconv4x4s2_fwd: Cout must be a multiple of 16 bytes");
  POSU_REQUIRE(static_cast<long long>(N) * 4 * H * W * Cout * cm_of(dtype) < (1LL << 31),
               "posu_deconv4x4s2_fwd: output too large");
  POSU_REQUIRE(params_aligned(scale, shift), "posu_deconv4x4s2_fwd: scale / shift must be 16-byte aligned");
  ConvGeom g = base_geom(x, N, H, W, C, w, Cout, dtype);
  g.scale = scale;
  g.shift = shift;
  g.y = y;
  g.Ho = H;
  g.Wo = W;
  g.M = N * H * W;
  g.K = 4 * g.C;
  g.Kpad = round_up(g.K, bk_of(dtype));
  g.KH = 2;
  g.KW = 2;
  g.relu = relu;
  g.deconv = 1;
  g.out_H = 2 * H;
  g.out_W = 2 * W;
  return dispatch<false>(dtype, g, 4, stream, "posu_deconv4x4s2_fwd", tile);
}

extern "C" int posu_deconv4x4s2_head_fwd(int dtype, const void* x, int N, int H, int W, int C, const void* w,
                                         int Cout, const float* scale, const float* shift, void* y, const void* hw,
                                         const void* hw_lo, int J, const float* hbias, float* hm, void* stream) {
  if (int st = common_checks(dtype, x, w, hm, N, H, W, C, Cout, "posu_deconv4x4s2_head_fwd")) return st;
  POSU_REQUIRE(hw && Cout == 256 && J > 0 && J <= 16,
               "posu_deconv4x4s2_head_fwd: needs Cout == 256, 0 < J <= 16 and head weights");
  POSU_REQUIRE(dtype != POSU_F16X3 || hw_lo, "posu_deconv4x4s2_head_fwd: split fp16 needs hw_lo");
  POSU_REQUIRE(((reinterpret_cast<size_t>(hw) | reinterpret_cast<size_t>(hw_lo)) & 15) == 0,
               "posu_deconv4x4s2_head_fwd: hw / hw_lo must be 16-byte aligned");
  POSU_REQUIRE(params_aligned(scale, shift), "posu_deconv4x4s2_head_fwd: scale / shift must be 16-byte aligned");
  ConvGeom g = base_geom(x, N, H, W, C, w, Cout, dtype);
  g.scale = scale;
  g.shift = shift;
  g.y = y;
  g.Ho = H;
  g.Wo = W;
  g.M = N * H * W;
  g.K = 4 * g.C;
  g.Kpad = round_up(g.K, bk_of(dtype));
  g.KH = 2;
  g.KW = 2;
  g.relu = 1;
  g.deconv = 1;
  g.out_H = 2 * H;
  g.out_W = 2 * W;
  g.hw = hw;
  g.hw_lo = (dtype == POSU_BF16 || dtype == POSU_F16 || dtype == POSU_F16X3) ? hw_lo : nullptr;  // f32: exact
  g.hbias = hbias;
  g.hm = hm;
  g.J = J;
  g.hkp = round_up(Cout, bk_of(dtype));
  return dispatch<false>(dtype, g, 4, stream, "posu_deconv4x4s2_head_fwd");
}

extern "C" int posu_head1x1_nchw_fwd(int dtype, const void* x, int N, int H, int W, int C, const void* w,
                                     int Cout, const float* bias, float* y, void* stream) {
  if (int st = common_checks(dtype, x, w, y, N, H, W, C, Cout, "posu_head1x1_nchw_fwd")) return st;
  ConvGeom g = base_geom(x, N, H, W, C, w, Cout, dtype);
  g.shift = bias;
  g.y = y;
  g.Ho = H;
  g.Wo = W;
  g.M = N * H * W;
  g.K = g.C;
  g.Kpad = round_up(g.K, bk_of(dtype));
  g.out_H = H;
  g.out_W = W;
  g.mode = 1;
  return dispatch<false>(dtype, g, 1, stream, "posu_head1x1_nchw_fwd");
}

// Data gradient of a KHxKW / stride / pad convolution x[N,H,W,Cin] -> y[N,Ho,Wo,Cout]:
// dx = conv(dy, W flipped and transposed, pad K-1-pad) over dy, read as its
// zero-upsampled image when stride == 2 (g.up), so strided layers run through the same
// MFMA kernel as the forward.  `residual` (optional, [N,H,W,Cin]) is added in the
// epilogue: the identity-branch gradient of a residual block.
extern "C" int posu_conv2d_dgrad_tile(int dtype, const void* dy, int N, int Ho, int Wo, int Cout, const void* wt,
                                      int Cin, int KH, int KW, int stride, int pad, const void* residual, void* dx,
                                      int H, int W, int tile, void* stream);

extern "C" int posu_conv2d_dgrad(int dtype, const void* dy, int N, int Ho, int Wo, int Cout, const void* wt,
                                 int Cin, int KH, int KW, int stride, int pad, const void* residual, void* dx, int H,
                                 int W, void* stream) {
  return posu_conv2d_dgrad_tile(dtype, dy, N, Ho, Wo, Cout, wt, Cin, KH, KW, stride, pad, residual, dx, H, W, -1,
                                stream);
}

extern "C" int posu_conv2d_dgrad_tile(int dtype, const void* dy, int N, int Ho, int Wo, int Cout, const void* wt,
                                      int Cin, int KH, int KW, int stride, int pad, const void* residual, void* dx,
                                      int H, int W, int tile, void* stream) {
  POSU_REQUIRE(dtype != POSU_F16X3, "posu_conv2d_dgrad: the split dtype is inference-only");
  POSU_REQUIRE(tile_ok(dtype, tile), tile_error("posu_conv2d_dgrad: unknown tile configuration", dtype));
  if (int st = common_checks(dtype, dy, wt, dx, N, Ho, Wo, Cout, Cin, "posu_conv2d_dgrad")) return st;
  POSU_REQUIRE(Cin % (16 / esz_of(dtype)) == 0, "posu_conv2d_dgrad: Cin must be a multiple of 16 bytes");
  POSU_REQUIRE(stride == 1 || stride == 2, "posu_conv2d_dgrad: stride 1 or 2");
  POSU_REQUIRE(KH > 0 && KW > 0 && pad >= 0 && pad < KH && pad < KW, "posu_conv2d_dgrad: bad window");
  POSU_REQUIRE(H > 0 && W > 0 && Ho == (H + 2 * pad - KH) / stride + 1 && Wo == (W + 2 * pad - KW) / stride + 1,
               "posu_conv2d_dgrad: H/W do not produce Ho/Wo under this window");
  POSU_REQUIRE(static_cast<long long>(N) * H * W * Cin < (1LL << 31), "posu_conv2d_dgrad: output too large");
  ConvGeom g = base_geom(dy, N, Ho, Wo, Cout, wt, Cin, dtype);
  g.res = residual;
  g.y = dx;
  if (KH == 1 && KW == 1 && pad == 0 && stride == 2 && residual == dx) {
    // 1x1 / stride 2, accumulated in place: dx[2i][2j] += dy[i][j] W^T, the other pixels keep
    // the residual -- a GEMM over dy's pixels instead of the zero-upsampled grid (4x fewer MACs)
    g.Ho = Ho;
    g.Wo = Wo;
    g.M = N * Ho * Wo;
    g.K = Cout;
    g.Kpad = round_up(g.K, bk_of(dtype));
    g.KH = 1;
    g.KW = 1;
    g.stride = 1;
    g.pad_h = 0;
    g.pad_w = 0;
    g.up = 0;
    g.out_H = H;
    g.out_W = W;
    g.ostride = 2;
    return dispatch<false>(dtype, g, 1, stream, "posu_conv2d_dgrad", tile);
  }
  g.Ho = H;
  g.Wo = W;
  g.M = N * H * W;
  g.K = KH * KW * Cout;
  g.Kpad = round_up(g.K, bk_of(dtype));
  g.KH = KH;
  g.KW = KW;
  g.stride = 1;
  g.pad_h = KH - 1 - pad;
  g.pad_w = KW - 1 - pad;
  g.up = stride == 2 ? 1 : 0;
  g.out_H = H;
  g.out_W = W;
  return dispatch<false>(dtype, g, 1, stream, "posu_conv2d_dgrad", tile);
}

// Plain GEMM on the conv kernel (1x1 window over M "pixels" of K channels):
//   out[blk][m][j] = sum_k x[m][k] * wt[blk * vblk + j][k]   (f32, blk = column / vblk)
// x: [M][K] dtype, K % 64 == 0 and a power of two; wt: packed [round_up(Ncol, 64)][K]
// dtype.  Used by the cross-view Aggregation (ChannelWiseFC, multiview_pose_resnet.py
// :16-58): the V(V-1) per-pair [HW x HW] matrices are one block matrix, so all target
// views come out of one launch, view-major.
extern "C" int posu_gemm_rows_f32(int dtype, const void* x, int M, int K, const void* wt, int Ncol, int vblk,
                                  float* out, void* stream) {
  POSU_REQUIRE(dtype != POSU_F16X3, "posu_gemm_rows_f32: the split dtype is not supported");
  if (int st = common_checks(dtype, x, wt, out, M, 1, 1, K, Ncol, "posu_gemm_rows_f32")) return st;
  POSU_REQUIRE(K % bk_of(dtype) == 0, "posu_gemm_rows_f32: K must be a multiple of the K-tile");
  POSU_REQUIRE(vblk > 0 && vblk % 8 == 0 && Ncol % vblk == 0, "posu_gemm_rows_f32: vblk must divide Ncol (x8)");
  ConvGeom g = base_geom(x, M, 1, 1, K, wt, Ncol, dtype);
  g.y = out;
  g.Ho = 1;
  g.Wo = 1;
  g.M = M;
  g.K = K;
  g.Kpad = K;
  g.out_H = 1;
  g.out_W = 1;
  g.mode = 2;
  g.vblk = vblk;
  return dispatch<false>(dtype, g, 1, stream, "posu_gemm_rows_f32");
}
