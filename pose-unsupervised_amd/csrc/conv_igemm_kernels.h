// Device side of the implicit-GEMM convolution (conv_igemm.hip holds the overview, the tile
// table and the entry points): the launch geometry, the A-operand gather, the fragment-read +
// MFMA step and the output-pixel decode that both kernels share, then conv_igemm_kernel (one
// block per tile) and conv_persist_kernel (one block per run of tiles).
#pragma once
#include <type_traits>

#include "gemm_common.h"

// timing ablations of the staggered loop (tools/igemm_ablations.sh; results wrong): bit 1 no
// MFMA, 2 no vmcnt wait, 4 no operand DMA, 8 no LDS fragment reads, 16 no epilogue, 32 no head
// reduction / stores
#ifndef POSU_IG_ABLATE
#define POSU_IG_ABLATE 0
#endif

namespace posu {
namespace {

struct ConvGeom {
  const void* x;
  const void* x2;  // DUAL: second 1x1 source
  const void* w;
  const float* scale;
  const float* shift;
  const void* res;
  void* y;
  int N, H, W, C, logC;
  int H2, W2, C2, stride2, K1;  // DUAL: source-2 geometry, K offset where it starts
  int Ho, Wo, M;                // launch grid: rows = N*Ho*Wo
  int Cout, CoutPad, K, Kpad;
  int KH, KW, stride, pad_h, pad_w;
  int relu;
  int up;            // 1: the input is read as its zero-upsampled image u[2i] = x[i], u[odd] = 0
                     //    (data gradient of a stride-2 convolution as a stride-1 one)
  int deconv;        // blockIdx.z = parity class
  int ostride;       // > 1: output pixel (oy, ox) is written at (ostride oy, ostride ox) of out_H x out_W
                     //      (data gradient of a 1x1 / stride-2 convolution, accumulated in place)
  int out_H, out_W;  // output tensor spatial dims
  int mode;          // 0: NHWC out (dtype), 1: NCHW f32 out, 2: f32 rows blocked by vblk columns
  int vblk;          // mode 2: out[(co / vblk)][m][co % vblk] (view-major heatmaps of a GEMM)
  // fused 1x1 head (mode 0, Cout == 256): hm[n][j][pix] = bias[j] + sum_c hw[j][c] relu(out[c])
  const void* hw;    // packed head weight [>= 16 rows][hkp] (dtype)
  const void* hw_lo;  // NULL, or the head weight's rounding residual (w - hw, rounded, same layout):
                      // the split-precision head (hi + lo operands on both sides, three MFMAs)
  const float* hbias;
  float* hm;
  int J, hkp;
  int mtiles, ntiles;
  int warm;          // > 0: workgroups 0 .. warm-1 touch the weights at their start (kernel comment)
  long long wseg;    // the weight tensor's 64-B segments (all parity classes)
};

// Weight warm-up (round 5, gemm_common.h warm_issue): layer4's 3x3 ran 59.4 us with its weights
// coming from HBM against 49.7 us with them re-read beforehand (tools/tile_micro.py --flush --touch,
// profiles/r05/tile_cold_touch_r5v.txt); with the warm-up the network ran 2.355-2.363 vs
// 2.405-2.413 ms (profiles/r05/weight_warmup_ab_r5y.txt).  (A side-stream prefetch launch inside
// the captured graph lost: its launches serialised with the network's, prefetch_ab_r5x.txt.)

template <int BM, int BN, int S>
constexpr int ring_bytes() {
  return S * (BM + BN) * 128;
}
// rows per epilogue pass: the f32 [rows][BN+4] staging tile must fit in the ring
template <int BM, int BN, int S>
constexpr int pass_rows() {
  return (BM * (BN + 4) * 4 <= ring_bytes<BM, BN, S>())         ? BM
         : ((BM / 2) * (BN + 4) * 4 <= ring_bytes<BM, BN, S>()) ? BM / 2
                                                                 : BM / 4;
}

// residual-add launches with at most this many K-tiles load their residual before the
// operand fetch (direct epilogue), so its HBM latency overlaps the main loop
constexpr int kEarlyNK = 8;

// BM x BN tile, NW waves (NT = 64*NW threads) in a WGM x (NW/WGM) grid, S-slot ring.
// SG: eight-wave tiles with waves 4-7 staggered by half a K-tile (two-slot ring).
// HD: the instance that carries the fused 1x1 head in its epilogue (256x256 eight-wave tiles
// only).  Its registers (head accumulators and weight fragments) made the 256x256 instance
// spill 36 VGPRs to scratch in every launch until round 4, head or not; the plain instances
// no longer hold that code (228 VGPRs, no scratch).
// KS (round 5): eight waves as two K groups of four -- the K-tiles come in pairs (two LDS sub-slots
// per ring slot), group g multiplies K-tile 2t + g of every pair over the WHOLE BM x BN tile, and
// the two partial sums meet in LDS at the end (each group adds the other's half of the m-tiles and
// stores that half).  Per wave 64 x 64 (TM = TN = 4) instead of the 64 x 32 of the eight-wave
// 128 x 128 tile: half the LDS fragment reads per MFMA, for grids of few tiles (layer4's M = 8192
// convs: 256 tiles of 128 x 128, one per CU).  The K order differs from the other tiles (the even
// and the odd K-tiles summed apart, then added), so KS results are not bit-identical to them.
template <typename T_, int BM_, int BN_, int NW_, int WGM_, int S_, bool DUAL_, bool SG_ = false, bool HD_ = false,
          bool KS_ = false>
struct TileCfg {
  using T = T_;
  using O = Op<T>;
  static constexpr int BM = BM_, BN = BN_, NW = NW_, WGM = WGM_, S = S_;
  static constexpr bool DUAL = DUAL_, SG = SG_, HD = HD_, KS = KS_;
  static constexpr int NT = NW * 64;
  static constexpr int E = O::E;
  static constexpr int ES = static_cast<int>(sizeof(T));
  // split fp16: K-tiles of [hi 32 | lo 32] halves, three MFMAs per K-tile and fragment pair;
  // outputs / residuals are (hi, lo) pairs, ocs halves per output pixel
  static constexpr bool SPL = O::SPLIT;
  // (round 6: the split dtype staggers too -- the lagging waves hold a K-tile's third product, hi(w).lo(x))
  static constexpr int BK = 8 * E;                   // 128-byte LDS rows
  static_assert(!KS || (NW == 8 && S == 2 && !SG && !HD && E == 8), "K groups: eight waves, two slots of pairs");
  static constexpr int NWG = KS ? NW / 2 : NW;       // waves per K group
  static constexpr int SL = KS ? 2 * S : S;          // LDS K-tile slots (KS: a pair per ring slot)
  static constexpr int WGN = NWG / WGM;              // wave grid WGM x WGN (of a K group)
  static constexpr int WTM = BM / WGM, WTN = BN / WGN;
  static constexpr int TM = WTM / 16, TN = WTN / 16;
  static constexpr int ROWS = NW * 8;                // LDS rows filled per DMA round (1 KiB per wave)
  static constexpr int RA = BM / ROWS, RB = BN / ROWS;
  static constexpr int ND = RA + RB;                 // DMA instructions per thread per K-tile
  static constexpr int A_BYTES = BM * 128, STAGE = (BM + BN) * 128;
  static constexpr int PR = pass_rows<BM, BN, SL>();
  static constexpr bool PRELOAD = TM + TN <= 8;  // both k-steps' fragments fit the VGPR budget
  static_assert(S >= 1 && S <= 4, "1..4 stages");
  static_assert(ND * (S - 2) < 64, "vmcnt range");
  static_assert(PR * (BN + 4) * 4 <= ring_bytes<BM, BN, SL>(), "epilogue staging must fit in the ring");
  static_assert(RA * ROWS == BM && RB * ROWS == BN, "tile rows must be a multiple of 8 * waves");
};

// ---- GEMM row m -> pixel (n, oy, ox) of the launch grid -> where that pixel lies in the output
// tensor: (osc oy + oy_off, osc ox + ox_off) of out_H x out_W (deconv parity classes, in-place
// strided dgrad; osc = 1 and no offsets otherwise)
struct OutMap {
  int HoWo, Wo, out_H, out_W, osc, oy_off, ox_off;
  struct Pix {
    int n, y, x;
  };
  __device__ __forceinline__ Pix grid(int m) const {
    const int n = m / HoWo, rem = m - n * HoWo;
    const int oy = rem / Wo, ox = rem - oy * Wo;
    return {n, oy, ox};
  }
  __device__ __forceinline__ Pix pixel(int m) const {
    const Pix p = grid(m);
    return {p.n, p.y * osc + oy_off, p.x * osc + ox_off};
  }
  // element offset of row m's output pixel in an NHWC tensor of `per` elements per pixel
  template <typename I = size_t>
  __device__ __forceinline__ I nhwc(int m, int per) const {
    const Pix p = pixel(m);
    return (static_cast<I>(p.n * out_H + p.y) * out_W + p.x) * per;
  }
  // its index inside image n's out_H x out_W plane (NCHW heatmaps)
  __device__ __forceinline__ int plane(int m, int& n) const {
    const Pix p = pixel(m);
    n = p.n;
    return p.y * out_W + p.x;
  }
};

// what a deconv parity class (py, px) = (cls >> 1, cls & 1) changes: the window origin, the output
// pixel map and the weight slice (element offset); cls = 0 of a launch without classes changes nothing
struct ClassGeom {
  int pad_h, pad_w;
  size_t wofs;
  OutMap out;
};
__device__ __forceinline__ ClassGeom class_geom(const ConvGeom& g, int cls) {
  ClassGeom c{g.pad_h, g.pad_w, 0, {g.Ho * g.Wo, g.Wo, g.out_H, g.out_W, g.ostride > 1 ? g.ostride : 1, 0, 0}};
  if (g.deconv) {
    const int py = cls >> 1, px = cls & 1;
    c.pad_h = 1 - py;
    c.pad_w = 1 - px;
    c.out.oy_off = py;
    c.out.ox_off = px;
    c.out.osc = 2;
    c.wofs = static_cast<size_t>(cls) * g.CoutPad * g.Kpad;
  }
  return c;
}

// ---- A-operand gather and weight rows of one tile, as LDS-DMA source offsets.  One
// buffer_load_dwordx4 ... lds per wave writes 1 KiB = 8 LDS rows x 8 chunks, lane l at byte 16*l:
// row (tid >> 3) + ROWS*i, physical chunk tid & 7.  The XOR swizzle of the fragment reads is
// applied on the SOURCE: that lane fetches logical chunk cL = (tid & 7) ^ ((row >> 1) & 7), which
// is the same for every i because ROWS*i does not touch bits 1..3 of the row.
// init() holds what the launch fixes, set_tile() the per-row state of tile (m0, n0) of a parity
// class, a_offsets() / b_offsets() hand K-tile kt's RA pixel-row and RB weight-row byte offsets to
// `put(i, offset)` (kOOB: the DMA writes zeros); second() says which DUAL source the RA address.
template <typename C>
struct Gather {
  using T = typename C::T;
  static constexpr int E = C::E, ES = C::ES, BK = C::BK, ROWS = C::ROWS, RA = C::RA, RB = C::RB;
  u32x4 xrs, x2rs, wrs;
  int cL, wbrow;  // this lane's logical chunk; weight row offset (elements) for i = 0
  // K-tile -> (kh, kw, ci) of this thread's chunk.  Three regimes:
  //  tap_uniform: C % BK == 0, one tap per K-tile (all 3x3 / 1x1 / deconv layers);
  //  row_uniform: KW*C == BK, one kernel row per K-tile (space-to-depth stem);
  //  generic    : per-chunk tap decode (C = 8 direct stem, f32 stem).
  bool tap_uniform, fast_gather, row_fast, row_uniform;
  int kwl, cil;                 // row_uniform: this lane's (kw, ci) column
  int hb[RA], wb[RA], nb[RA];   // generic window gather
  int o1[RA], o2[RA];           // DUAL: byte offsets of the two 1x1 sources
  int rbase[RA];                // row_fast: window row origin + this lane's (kw, ci) column
  bool wok[RA];
  int pbase[RA];                // element offset of row i's window origin + this lane's channel chunk

  __device__ __forceinline__ void init(const ConvGeom& g, int tid) {
    xrs = make_srd(g.x, g.N * g.H * g.W * g.C * ES);
    x2rs = xrs;
    if constexpr (C::DUAL) x2rs = make_srd(g.x2, g.N * g.H2 * g.W2 * g.C2 * ES);
    wrs = xrs;
    wbrow = 0;
    cL = (tid & 7) ^ ((tid >> 4) & 7);
    tap_uniform = (g.C % BK) == 0;
    fast_gather = tap_uniform && g.up == 0;
    row_uniform = !tap_uniform && g.KW * g.C == BK;
    row_fast = row_uniform && g.up == 0;
    kwl = (cL * E) >> g.logC;
    cil = (cL * E) & (g.C - 1);
  }

  __device__ __forceinline__ void set_tile(const ConvGeom& g, int tid, int m0, int n0, const ClassGeom& cg) {
    wrs = make_srd(reinterpret_cast<const T*>(g.w) + cg.wofs, g.CoutPad * g.Kpad * ES);
    wbrow = (n0 + (tid >> 3)) * g.Kpad + cL * E;
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      const int m = m0 + (tid >> 3) + ROWS * i;
      if (m < g.M) {
        const OutMap::Pix p = cg.out.grid(m);
        hb[i] = p.y * g.stride - cg.pad_h;
        wb[i] = p.x * g.stride - cg.pad_w;
        nb[i] = p.n * g.H * g.W * g.C;
        if constexpr (C::DUAL) {
          o1[i] = (m * g.C + cL * E) * ES;
          o2[i] = (((p.n * g.H2 + p.y * g.stride2) * g.W2 + p.x * g.stride2) * g.C2 + cL * E) * ES;
        }
      } else {
        hb[i] = -(1 << 28);
        wb[i] = 0;
        nb[i] = 0;
        if constexpr (C::DUAL) {
          o1[i] = kOOB;
          o2[i] = kOOB;
        }
      }
      wok[i] = static_cast<unsigned>(wb[i] + kwl) < static_cast<unsigned>(g.W);
      // unsigned: rows past M carry a huge negative hb (never dereferenced)
      rbase[i] = static_cast<int>(static_cast<unsigned>(nb[i]) +
                                  (static_cast<unsigned>(hb[i]) * g.W + static_cast<unsigned>(wb[i] + kwl)) * g.C +
                                  cil);
      pbase[i] = static_cast<int>(static_cast<unsigned>(nb[i]) +
                                  (static_cast<unsigned>(hb[i]) * g.W + static_cast<unsigned>(wb[i])) * g.C + cL * E);
    }
  }

  __device__ __forceinline__ bool second(const ConvGeom& g, int kt) const { return C::DUAL && kt * BK >= g.K1; }

  template <typename F>
  __device__ __forceinline__ void a_offsets(const ConvGeom& g, int kt, F&& put) const {
    const int kbase = kt * BK;
    if constexpr (C::DUAL) {
      const bool first = kbase < g.K1;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const int o = first ? o1[i] : o2[i];
        put(i, o == kOOB ? kOOB : o + (first ? kbase : kbase - g.K1) * ES);
      }
    } else if (fast_gather) {
      // one tap per K-tile, no zero-upsampling: row base + a wave-uniform tap offset
      const int tap = kbase >> g.logC;
      const int th = tap / g.KW, tw = tap - th * g.KW;
      const int toff = (th * g.W + tw) * g.C + (kbase & (g.C - 1));
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const bool ok = static_cast<unsigned>(hb[i] + th) < static_cast<unsigned>(g.H) &&
                        static_cast<unsigned>(wb[i] + tw) < static_cast<unsigned>(g.W);
        put(i, ok ? (pbase[i] + toff) * ES : kOOB);
      }
    } else if (row_fast) {
      // one kernel row per K-tile (space-to-depth stem): lane column fixed per row
      const int roff = kt * g.W * g.C;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const bool ok = wok[i] && static_cast<unsigned>(hb[i] + kt) < static_cast<unsigned>(g.H);
        put(i, ok ? (rbase[i] + roff) * ES : kOOB);
      }
    } else {
      int kh, kw, ci;
      bool kvalid = true;
      if (tap_uniform) {
        const int tap = kbase >> g.logC;
        kh = tap / g.KW;
        kw = tap - kh * g.KW;
        ci = (kbase & (g.C - 1)) + cL * E;
      } else if (row_uniform) {
        kh = kt;
        kw = kwl;
        ci = cil;
      } else {
        const int k = kbase + cL * E;
        const int tap = k >> g.logC;
        kh = tap / g.KW;
        kw = tap - kh * g.KW;
        ci = k & (g.C - 1);
        kvalid = k < g.K;
      }
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const int hl = hb[i] + kh, wl = wb[i] + kw;
        const int hi = hl >> g.up, wi = wl >> g.up;
        const bool ok = kvalid && ((hl | wl) & g.up) == 0 && static_cast<unsigned>(hi) < static_cast<unsigned>(g.H) &&
                        static_cast<unsigned>(wi) < static_cast<unsigned>(g.W);
        put(i, ok ? (nb[i] + (hi * g.W + wi) * g.C + ci) * ES : kOOB);
      }
    }
  }

  template <typename F>
  __device__ __forceinline__ void b_offsets(const ConvGeom& g, int kt, F&& put) const {
#pragma unroll
    for (int i = 0; i < RB; ++i) put(i, (wbrow + ROWS * i * g.Kpad + kt * BK) * ES);
  }
};

// ---- fragment reads and MFMAs over one LDS K-tile.  Operands are swapped (A = weights, B =
// pixels), so a lane's accumulator holds 4 consecutive output channels of one pixel, staged into
// LDS with one 16-B write.
// N fragments of logical chunk c from the 16-row MFMA tiles at rows row0, row0 + 16, ... of an LDS
// operand tile (row0 = the wave's first tile row + the lane's r16)
template <int N>
__device__ __forceinline__ void read_frags(const char* tile, int row0, int c, uint4 (&f)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) f[i] = *reinterpret_cast<const uint4*>(tile + swz(row0 + i * 16, c));
}

struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};

// acc[i][j] += w[j] . x[i] for every fragment pair; hook(f0 + i * TN + j) runs after each MFMA
template <typename O, int TM, int TN, typename H = NoHook>
__device__ __forceinline__ void mma_all(f32x4 (&acc)[TM][TN], const uint4 (&x)[TM], const uint4 (&w)[TN], int f0 = 0,
                                        H&& hook = H{}) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      O::mma(acc[i][j], w[j], x[i]);
      hook(f0 + i * TN + j);
    }
}

// one K-tile at As (pixel rows, the weight rows A_BYTES behind): arow / brow are the wave's first
// pixel / weight tile row + r16, q the lane's chunk within a k-step
template <typename C, typename H = NoHook>
__device__ __forceinline__ void mma_ktile(const char* As, int arow, int brow, int q, f32x4 (&acc)[C::TM][C::TN],
                                          H&& hook = H{}) {
  using O = typename C::O;
  constexpr int TM = C::TM, TN = C::TN;
  const char* Bs = As + C::A_BYTES;
  if constexpr (C::SPL) {
    // k-step 0 = the hi halves, k-step 1 = the lo halves of the same 32 k: w.x as
    // hi.hi + lo(w).hi(x) + hi(w).lo(x); at most TM + 2 TN fragments live
    uint4 x0[TM], w0[TN];
    read_frags(Bs, brow, q, w0);
    read_frags(As, arow, q, x0);
    mma_all<O>(acc, x0, w0, 0, hook);
    {
      uint4 w1[TN];
      read_frags(Bs, brow, 4 + q, w1);
      mma_all<O>(acc, x0, w1, TM * TN, hook);
    }
    {
      uint4 x1[TM];
      read_frags(As, arow, 4 + q, x1);
      mma_all<O>(acc, x1, w0, 2 * TM * TN, hook);
    }
  } else if constexpr (C::PRELOAD) {
    // both k-steps' fragments first: the MFMAs then run back to back while the
    // second half's reads land, instead of stalling on them mid-tile
    uint4 af[2][TM], bfr[2][TN];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      read_frags(Bs, brow, 4 * cb + q, bfr[cb]);
      read_frags(As, arow, 4 * cb + q, af[cb]);
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) mma_all<O>(acc, af[cb], bfr[cb], cb * TM * TN, hook);
  } else {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      uint4 af[TM], bfr[TN];
      read_frags(As, arow, 4 * cb + q, af);
      read_frags(Bs, brow, 4 * cb + q, bfr);
      mma_all<O>(acc, af, bfr, cb * TM * TN, hook);
    }
  }
}

// ---- one block per BM x BN tile (TileCfg explains the parameters): tile decode and gather set-up,
// residual prefetch, one of four main loops, one of five epilogues.  The loops and epilogues stand
// in the kernel body itself, not in functions of their own: as separately optimised functions
// (members of a tile struct, or lambdas) they cost registers and scratch -- the K-group hand-off
// and the 256x64 DUAL tile went to scratch (48-240 B per lane), the 256x256 ring spilled 34 VGPRs
// and several f32 tiles lost a wave per SIMD -- because the optimiser then sees the accumulators
// as memory behind a pointer before it inlines.
template <typename T, int BM, int BN, int NW, int WGM, int S, bool DUAL, bool SG = false, bool HD = false,
          bool KS = false>
__global__ __launch_bounds__(NW * 64) void conv_igemm_kernel(ConvGeom g) {
  using C = TileCfg<T, BM, BN, NW, WGM, S, DUAL, SG, HD, KS>;
  __shared__ __attribute__((aligned(16))) char smem[ring_bytes<BM, BN, C::SL>()];
  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) char*)smem));
  using O = typename C::O;
  constexpr int NT = C::NT, E = C::E;
  constexpr int NWG = C::NWG, WGN = C::WGN, WTM = C::WTM, WTN = C::WTN, TM = C::TM, TN = C::TN;
  constexpr int ND = C::ND, A_BYTES = C::A_BYTES, STAGE = C::STAGE, PR = C::PR;
  constexpr bool SPL = C::SPL;
  // Early residual prefetch (short-K Bottleneck tails): the residual chunks, in the direct
  // epilogue's lane layout, are loaded before the first operand DMA, so their HBM latency
  // overlaps the operand fetch instead of following the main loop.
  constexpr bool EARLY = E == 8 && TN % 2 == 0 && TM * TN <= 16 && !SPL && !KS;
  constexpr int ETM = EARLY ? TM : 1, ETP = EARLY ? TN / 2 : 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int grp = KS ? wid / NWG : 0, wl = KS ? wid % NWG : wid;   // K group, wave in the group
  const int wm = wl / WGN, wn = wl % WGN;
  const int r16 = lane & 15, q = lane >> 4;
  const unsigned wid_u = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(wid));
  // tile row of the wave's m-tile i / tile column of its n-tile j
  auto rowA = [&](int i) { return wm * WTM + i * 16; };
  auto colB = [&](int j) { return wn * WTN + j * 16; };

  // ---- tile decode and gather set-up
  // XCD-aware tile order: blocks b and b+8 share an XCD; give each XCD a
  // contiguous run of tiles so neighbouring tiles (same A rows) share its L2.
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
  // tile id -> (m-tile, [deconv parity class,] n-tile), n fastest; the 4 parity
  // classes of one m-tile are adjacent so their overlapping input windows are read
  // from the same XCD's L2 instead of once per class from HBM
  const int nt = wg % g.ntiles;
  const int rest = wg / g.ntiles;
  const int mt = g.deconv ? rest >> 2 : rest;
  const int m0 = mt * BM, n0 = nt * BN;
  const ClassGeom cg = class_geom(g, rest & 3);
  const OutMap om = cg.out;
  const int ocs = SPL ? 2 * g.Cout : g.Cout;  // elements per output pixel
  const int nk = g.Kpad / C::BK;
  Gather<C> ga;
  ga.init(g, tid);
  ga.set_tile(g, tid, m0, n0, cg);

  // acc[i][j]: rows = channels of n-tile j (16 per MFMA tile), cols = pixels of m-tile i;
  // lane holds channels 4q..4q+3 of pixel r16
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bool early;
  uint4 rve[ETM][ETP];
  unsigned wv[kWarmLoads];

  // element offset of the output pixel of m-tile i's row of this lane (row 0 where m is past M)
  auto out_pix = [&](int i, bool& mok) -> size_t {
    const int m = m0 + rowA(i) + r16;
    mok = m < g.M;
    return om.nhwc(mok ? m : 0, ocs);
  };

  auto prefetch_residual = [&]() -> void {
    early = EARLY && g.res && g.mode == 0 && !g.hm && nk <= kEarlyNK;
    if constexpr (EARLY) {
      if (early) {
        const T* __restrict__ rp = reinterpret_cast<const T*>(g.res);
#pragma unroll
        for (int i = 0; i < ETM; ++i) {
          bool mok;
          const size_t pix = out_pix(i, mok);
#pragma unroll
          for (int jp = 0; jp < ETP; ++jp) {
            const int co = n0 + colB(2 * jp + (q & 1)) + 8 * (q >> 1);
            rve[i][jp] = make_uint4(0, 0, 0, 0);
            if (mok && co < g.Cout) rve[i][jp] = *reinterpret_cast<const uint4*>(rp + pix + co);
          }
        }
      }
    }
  };

  // weight warm-up: this workgroup's segments requested now, consumed right after the first
  // K-tile DMAs are issued
  auto warm_start = [&]() -> void { warm_issue(wv, g.w, g.wseg, g.warm, NT); };
  auto warm_done = [&]() -> void { warm_use(wv); };

  // global -> LDS (async DMA) for K-tile kt into ring slot buf: exactly ND dma16 per thread
  auto dma_tile = [&](int kt, int buf) -> void {
    const unsigned As_ = lds0 + buf * STAGE + wid_u * 1024;
    const unsigned Bs_ = As_ + A_BYTES;
    const bool sec = ga.second(g, kt);
    ga.a_offsets(g, kt, [&](int i, int off) { dma16(sec ? ga.x2rs : ga.xrs, off, As_ + i * NW * 1024); });
    ga.b_offsets(g, kt, [&](int i, int off) { dma16(ga.wrs, off, Bs_ + i * NW * 1024); });
  };
  auto compute = [&](int buf) -> void {
    mma_ktile<C>(smem + buf * STAGE, rowA(0) + r16, colB(0) + r16, q, acc);
  };

  // timing ablation: no epilogue (results wrong)
  auto drop_acc = [&]() -> void {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(acc[i][j]));
  };

  // ---- epilogues
  // the lane's values of the n-tile pair jp of m-tile i: v_permlane16_swap pairs the n-tiles
  // (j, j+1) so that every lane holds 8 consecutive channels (16-B stores, half the store
  // instructions): lane (r16, q) gets n-tile j + (q & 1), channels 8 * (q >> 1) .. + 7 of pixel r16
  auto pair8 = [&](int i, int jp, float* v) -> void {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][2 * jp][e]),
                                                       __float_as_uint(acc[i][2 * jp + 1][e]), false, false);
      v[e] = __uint_as_float(sw[0]);
      v[4 + e] = __uint_as_float(sw[1]);
    }
  };
  // the BN parameters of the 8 consecutive channels from cp, all inside Cout or all past it (Cout is
  // a multiple of 8): two 16-B loads per parameter instead of eight 4-B ones
  auto params8 = [&](int cp, float* sc8, float* sh8) -> void {
    const bool in = cp < g.Cout;
    float4 s0 = make_float4(1.f, 1.f, 1.f, 1.f), s1 = s0, h0 = make_float4(0.f, 0.f, 0.f, 0.f), h1 = h0;
    if (in && g.scale) {
      s0 = *reinterpret_cast<const float4*>(g.scale + cp);
      s1 = *reinterpret_cast<const float4*>(g.scale + cp + 4);
    }
    if (in && g.shift) {
      h0 = *reinterpret_cast<const float4*>(g.shift + cp);
      h1 = *reinterpret_cast<const float4*>(g.shift + cp + 4);
    }
    sc8[0] = s0.x; sc8[1] = s0.y; sc8[2] = s0.z; sc8[3] = s0.w;
    sc8[4] = s1.x; sc8[5] = s1.y; sc8[6] = s1.z; sc8[7] = s1.w;
    sh8[0] = h0.x; sh8[1] = h0.y; sh8[2] = h0.z; sh8[3] = h0.w;
    sh8[4] = h1.x; sh8[5] = h1.y; sh8[6] = h1.z; sh8[7] = h1.w;
  };
  // the BN parameters of the lane's 4 channels of every n-tile
  auto params4 = [&](float (&sc)[TN][4], float (&sh)[TN][4]) -> void {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = n0 + colB(j) + q * 4 + e;
        sc[j][e] = (co < g.Cout && g.scale) ? g.scale[co] : 1.f;
        sh[j][e] = (co < g.Cout && g.shift) ? g.shift[co] : 0.f;
      }
  };

  // the E values of chunk cc of staged row `row`
  constexpr int LD = BN + 4;
  auto staged_vals = [&](const float* Cs, int row, int cc, float* v) -> void {
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const float4 t4 = *reinterpret_cast<const float4*>(Cs + row * LD + cc * E + e);
      v[e] = t4.x;
      v[e + 1] = t4.y;
      v[e + 2] = t4.z;
      v[e + 3] = t4.w;
    }
  };

  prefetch_residual();
  warm_start();

  // ---- main loop, one of four
  if constexpr (KS) {
    // K-tile pairs: pair t in slots 2 (t & 1) and 2 (t & 1) + 1, DMA'd by all eight waves one pair
    // ahead; group g multiplies the pair's K-tile 2t + g (a missing last odd K-tile is skipped)
    const int np = (nk + 1) / 2;
    dma_tile(0, 0);
    if (1 < nk) dma_tile(1, 1);
    warm_done();
    for (int t = 0; t < np; ++t) {
      vm_wait<0>();
      __syncthreads();
      if (t + 1 < np) {
        const int b = 2 * ((t + 1) & 1);
        dma_tile(2 * t + 2, b);
        if (2 * t + 3 < nk) dma_tile(2 * t + 3, b + 1);
      }
      if (2 * t + grp < nk) compute(2 * (t & 1) + grp);
    }
    // the two groups' partial sums: group 0 keeps m-tiles 0 .. TM/2 - 1, group 1 the rest; each hands
    // the other its half through LDS (f32, lane-major) and adds the half it keeps (a + b == b + a)
    __syncthreads();  // every wave is done reading the ring
    constexpr int HT = TM / 2, PER = HT * TN * 64;   // f32x4 per wave's hand-off
    f32x4* xch = reinterpret_cast<f32x4*>(smem);
    auto give = [&](auto g0) {
      constexpr bool G0 = decltype(g0)::value;
#pragma unroll
      for (int i = 0; i < HT; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) xch[(G0 ? 0 : NWG) * PER + wl * PER + (i * TN + j) * 64 + lane] = acc[G0 ? HT + i : i][j];
    };
    auto take = [&](auto g0) {
      constexpr bool G0 = decltype(g0)::value;
#pragma unroll
      for (int i = 0; i < HT; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[G0 ? i : HT + i][j] += xch[(G0 ? NWG : 0) * PER + wl * PER + (i * TN + j) * 64 + lane];
    };
    if (grp == 0) give(std::true_type{});
    else give(std::false_type{});
    __syncthreads();
    if (grp == 0) take(std::true_type{});
    else take(std::false_type{});
  } else if constexpr (SG) {
    static_assert(S == 2 && NW == 8, "stagger: eight waves, two slots");
    // Stagger (two-slot ring, one barrier per K-tile): waves 4-7 run half a K-tile behind
    // waves 0-3 -- they keep the second k-step's fragments of K-tile t in registers and
    // issue its MFMAs after the next barrier, while waves 0-3 wait for their first
    // fragment reads; every read still happens before the barrier that frees its slot.
    const bool lag = wid_u >= 4;
    const int arow = rowA(0) + r16, brow = colB(0) + r16;
    uint4 hA[TM], hB[TN];
    auto read = [&](const char* As_, const char* Bs_, int cb, uint4 (&a)[TM], uint4 (&b)[TN]) {
      read_frags(As_, arow, 4 * cb + q, a);
      read_frags(Bs_, brow, 4 * cb + q, b);
    };
    auto mma = [&](const uint4 (&a)[TM], const uint4 (&b)[TN]) { mma_all<O>(acc, a, b); };
    constexpr int ABL = POSU_IG_ABLATE;
    auto mmx = [&](const uint4 (&a)[TM], const uint4 (&b)[TN]) {
      if constexpr (ABL & 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[i][0][0] += __builtin_bit_cast(float, a[i].x ^ b[i % TN].y);
      } else {
        mma(a, b);
      }
    };
    auto rdx = [&](const char* As_, const char* Bs_, int cb, uint4 (&a)[TM], uint4 (&b)[TN]) {
      if constexpr (ABL & 8) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = make_uint4(cb, i, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = make_uint4(j, cb, 0, 0);
      } else {
        read(As_, Bs_, cb, a, b);
      }
    };
    if constexpr (!(ABL & 4)) dma_tile(0, 0);
    warm_done();
    if (lag) __builtin_amdgcn_s_setprio(1);  // the lagging half wins issue arbitration (-2..-7 %)
    if constexpr (SPL) {
      // split fp16 (round 6): a K-tile's products are hi.hi and lo(w).hi(x) over the hi pixel
      // fragments, then hi(w).lo(x); the lagging waves keep the last one's operands (the lo pixel and
      // the hi weight fragments) and issue it after the next barrier, before the next K-tile's hi.hi
      // -- per accumulator the plain loop's sequence, so the results are bit-identical to it
      for (int kt = 0; kt < nk; ++kt) {
        vm_wait<0>();
        __syncthreads();
        if (kt + 1 < nk) dma_tile(kt + 1, (kt + 1) & 1);
        const char* As_ = smem + (kt & 1) * STAGE;
        const char* Bs_ = As_ + A_BYTES;
        if (lag && kt > 0) mma(hA, hB);
        uint4 af[TM], bfr[TN];
        read(As_, Bs_, 0, af, bfr);
        mma(af, bfr);
        {
          uint4 bl[TN];
          read_frags(Bs_, brow, 4 + q, bl);
          mma(af, bl);
        }
        read_frags(As_, arow, 4 + q, hA);
#pragma unroll
        for (int j = 0; j < TN; ++j) hB[j] = bfr[j];
        if (!lag) mma(hA, hB);
      }
    } else {
      for (int kt = 0; kt < nk; ++kt) {
        if constexpr (!(ABL & 2)) vm_wait<0>();
        __syncthreads();
        if constexpr (!(ABL & 4))
          if (kt + 1 < nk) dma_tile(kt + 1, (kt + 1) & 1);
        const char* As_ = smem + (kt & 1) * STAGE;
        const char* Bs_ = As_ + A_BYTES;
        uint4 af[TM], bfr[TN];
        if (lag && kt > 0) mmx(hA, hB);
        rdx(As_, Bs_, 0, af, bfr);
        mmx(af, bfr);
        rdx(As_, Bs_, 1, hA, hB);
        if (!lag) mmx(hA, hB);
      }
    }
    if (lag) mmx(hA, hB);
    if constexpr (ABL & 2) vm_wait<0>();
    __builtin_amdgcn_s_setprio(0);
  } else if constexpr (S == 1) {
    // single slot (short-K layers): a quarter of the LDS of a 2-slot ring, so more
    // blocks share a CU and one block's epilogue overlaps another's operand fetch
    for (int kt = 0; kt < nk; ++kt) {
      if (kt > 0) __syncthreads();  // every wave is done reading the slot
      dma_tile(kt, 0);
      if (kt == 0) warm_done();
      vm_wait<0>();
      __syncthreads();
      compute(0);
    }
  } else {
    // S-slot ring, DMA running S-1 K-tiles ahead; per K-tile one counted vmcnt
    // (the K-tile being consumed has landed, up to S-2 younger tiles stay in flight) and one
    // barrier (makes the DMA visible to every wave and retires the slot the next DMA
    // overwrites, which every wave finished reading in the previous iteration)
#pragma unroll
    for (int s = 0; s < S - 1; ++s)
      if (s < nk) dma_tile(s, s);
    warm_done();
    for (int kt = 0; kt < nk; ++kt) {
      const int ahead = min(S - 2, nk - 1 - kt);  // younger K-tiles in flight
      if (S >= 4 && ahead >= 2) vm_wait<ND * (S >= 4 ? 2 : 0)>();
      else if (S >= 3 && ahead >= 1) vm_wait<ND * (S >= 3 ? 1 : 0)>();
      else vm_wait<0>();
      __syncthreads();
      if (kt + S - 1 < nk) dma_tile(kt + S - 1, (kt + S - 1) % S);
      compute(kt % S);
    }
  }

  constexpr bool HEAD256 = HD && BM == 256 && BN == 256 && NW == 8 && WGM == 2 && C::E == 8;
  static_assert(!HD || HEAD256, "the fused head runs on the 2-byte 256x256 eight-wave tile");
  // ---- epilogue, one of five
  if constexpr (SG && (POSU_IG_ABLATE & 16)) {
    drop_acc();
  } else if constexpr (HEAD256) {
    // 256x256 tiles also carry the fused 1x1 head (pose_resnet.py:126-132, 203): each
    // wave's rounded outputs are already MFMA B fragments (8 consecutive channels of one
    // pixel per lane), so its partial heatmaps over its 64 channels are 2 MFMAs per m-tile;
    // the four column waves' partials are summed in LDS in a fixed order.
    // (the HD instance: launched only with g.hm set, no other epilogue)
    T* __restrict__ yp = reinterpret_cast<T*>(g.y);
    const T* __restrict__ rp = reinterpret_cast<const T*>(g.res);
    constexpr int TP = TN / 2;
    // fused head: pair jp outer, m-tile inner -- one pair's BN parameters and head fragments
    // are live at a time and each accumulator pair dies once consumed (the 256x256 head
    // instance spilled 38 VGPRs with m-tile outer); every hacc[i] still receives its MFMAs in
    // the same order (pair 0's, then pair 1's), so the heatmaps are unchanged
    const bool split = SPL || g.hw_lo != nullptr;  // the split dtype's head is always split
    const T* __restrict__ hwp = reinterpret_cast<const T*>(g.hw);
    const T* __restrict__ hwq = reinterpret_cast<const T*>(split ? g.hw_lo : g.hw);
    f32x4 hacc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) hacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool need_pix = yp != nullptr || rp != nullptr;
#pragma unroll
    for (int jp = 0; jp < TP; ++jp) {
      // 8 consecutive channels cp .. cp + 7 of this lane (all inside Cout or all past it)
      const int cp = n0 + colB(2 * jp + (q & 1)) + 8 * (q >> 1);
      const bool in = cp < g.Cout;
      float sc8[8], sh8[8];
      params8(cp, sc8, sh8);
      // joint r16's weights over this lane's 8 channels
      const size_t o = static_cast<size_t>(r16) * g.hkp + cp;
      const uint4 hw = *reinterpret_cast<const uint4*>(hwp + o);
      const uint4 hl = *reinterpret_cast<const uint4*>(hwq + o);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        bool mok = m0 + rowA(i) + r16 < g.M;
        size_t pix = 0;
        if (need_pix) pix = out_pix(i, mok);
        float v[8], r[8];
        pair8(i, jp, v);
        if constexpr (SPL) {
          uint4 rh = make_uint4(0, 0, 0, 0), rl = rh;
          if (rp && mok && in) {
            rh = *reinterpret_cast<const uint4*>(rp + pix + split_ch(cp));
            rl = *reinterpret_cast<const uint4*>(rp + pix + split_ch(cp) + 32);
          }
          join8(rh, rl, r);
        } else {
          uint4 rv = make_uint4(0, 0, 0, 0);
          if (rp && mok && in) rv = *reinterpret_cast<const uint4*>(rp + pix + cp);
          O::load_vals(rv, r);
        }
        affine8<false>(v, sc8, sh8);
        if (rp) add8<false>(v, r);
        if (g.relu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        const uint4 pk = O::store_vals(v);
        O::mma(hacc[i], hw, pk);  // rows = joints, cols = pixels
        uint4 pl = make_uint4(0, 0, 0, 0);
        if (split) {
          // the deconv output's rounding residual v - round(v) (exact in f32) rounded again: the
          // head sees v to 2 x the dtype's mantissa, its weights likewise (hi.hi + lo.hi + hi.lo)
          float vr[8], vl[8];
          O::load_vals(pk, vr);
#pragma unroll
          for (int e = 0; e < 8; ++e) vl[e] = v[e] - vr[e];
          pl = O::store_vals(vl);
          O::mma(hacc[i], hl, pk);
          O::mma(hacc[i], hw, pl);
        }
        if constexpr (SPL) {
          if (yp && mok) {
            *reinterpret_cast<uint4*>(yp + pix + split_ch(cp)) = pk;
            *reinterpret_cast<uint4*>(yp + pix + split_ch(cp) + 32) = pl;
          }
        } else {
          if (yp && mok) *reinterpret_cast<uint4*>(yp + pix + cp) = pk;
        }
      }
    }
    if constexpr (SG && (POSU_IG_ABLATE & 32)) {  // timing ablation: no head reduction / stores
#pragma unroll
      for (int i = 0; i < TM; ++i) asm volatile("" ::"v"(hacc[i]));
      return;
    }
    __syncthreads();  // the ring is no longer read: partial heatmaps [wn][joint][256 px]
    float* Hs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) Hs[(wn * 16 + 4 * q + e) * BM + rowA(i) + r16] = hacc[i][e];
    __syncthreads();
    const int HWo = g.out_H * g.out_W;
    for (int idx = tid; idx < g.J * BM; idx += NT) {
      const int j = idx / BM, pl = idx - j * BM;
      const int m = m0 + pl;
      if (m >= g.M) continue;
      float sum = g.hbias ? g.hbias[j] : 0.f;
#pragma unroll
      for (int w4 = 0; w4 < 4; ++w4) sum += Hs[(w4 * 16 + j) * BM + pl];
      int n;
      const int pixo = om.plane(m, n);
      g.hm[(static_cast<size_t>(n) * g.J + j) * HWo + pixo] = sum;
    }
  } else if (E == 8 && TN % 2 == 0 && g.mode == 0 && !g.hm) {
    // ---- direct epilogue (NHWC outputs): each lane stores its 4
    // consecutive channels of one pixel straight from the accumulators (BN, residual,
    // ReLU applied in registers) -- no LDS round trip, no barriers
    // 2-byte outputs: 8 consecutive channels per lane (pair8), 16-B stores
    T* __restrict__ yp = reinterpret_cast<T*>(g.y);
    const T* __restrict__ rp = reinterpret_cast<const T*>(g.res);
    constexpr int TP = TN / 2;
    int cop[TP];
    float sc[TP][8], sh[TP][8];
#pragma unroll
    for (int jp = 0; jp < TP; ++jp) {
      cop[jp] = n0 + colB(2 * jp + (q & 1)) + 8 * (q >> 1);
      params8(cop[jp], sc[jp], sh[jp]);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if (KS && (i < TM / 2) != (grp == 0)) continue;   // (wave-uniform) the other group's half
      bool mok;
      const size_t pix = out_pix(i, mok);
      uint4 rv[TP], rl[TP];
#pragma unroll
      for (int jp = 0; jp < TP; ++jp) {
        rv[jp] = make_uint4(0, 0, 0, 0);
        rl[jp] = rv[jp];
        if constexpr (SPL) {
          if (rp && mok && cop[jp] < g.Cout) {
            rv[jp] = *reinterpret_cast<const uint4*>(rp + pix + split_ch(cop[jp]));
            rl[jp] = *reinterpret_cast<const uint4*>(rp + pix + split_ch(cop[jp]) + 32);
          }
          continue;
        }
        if constexpr (EARLY) {
          if (early) {
            rv[jp] = rve[i][jp];
            continue;
          }
        }
        if (rp && mok && cop[jp] < g.Cout) rv[jp] = *reinterpret_cast<const uint4*>(rp + pix + cop[jp]);
      }
#pragma unroll
      for (int jp = 0; jp < TP; ++jp) {
        float v[8], r[8];
        pair8(i, jp, v);
        if constexpr (SPL) {
          join8(rv[jp], rl[jp], r);
        } else {
          O::load_vals(rv[jp], r);
        }
        affine8<false>(v, sc[jp], sh[jp]);
        if (rp) add8<false>(v, r);
        if (g.relu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if constexpr (SPL) {
          if (mok && cop[jp] < g.Cout) {
            uint4 h, l;
            split8(v, h, l);
            *reinterpret_cast<uint4*>(yp + pix + split_ch(cop[jp])) = h;
            *reinterpret_cast<uint4*>(yp + pix + split_ch(cop[jp]) + 32) = l;
          }
        } else {
          if (mok && cop[jp] < g.Cout) *reinterpret_cast<uint4*>(yp + pix + cop[jp]) = O::store_vals(v);
        }
      }
    }
  } else if (!SPL && g.mode == 0 && !g.hm) {
    // the lane's 4 channels of every n-tile as they are (f32: 16-B, 2-byte dtypes: 8-B stores)
    T* __restrict__ yp = reinterpret_cast<T*>(g.y);
    const T* __restrict__ rp = reinterpret_cast<const T*>(g.res);
    float sc[TN][4], sh[TN][4];
    params4(sc, sh);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      bool mok;
      const size_t pix = out_pix(i, mok);
      uint4 rv[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int co = n0 + colB(j) + q * 4;
        rv[j] = make_uint4(0, 0, 0, 0);
        if (rp && mok && co < g.Cout) {
          if constexpr (E == 4) {
            rv[j] = *reinterpret_cast<const uint4*>(rp + pix + co);
          } else {
            const uint2 r2 = *reinterpret_cast<const uint2*>(rp + pix + co);
            rv[j] = make_uint4(r2.x, r2.y, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int co = n0 + colB(j) + q * 4;
        if (!mok || co >= g.Cout) continue;
        float r[E], v[E];
        O::load_vals(rv[j], r);
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[i][j][e] * sc[j][e] + sh[j][e];
          if (rp) v[e] += r[e];
          if (g.relu) v[e] = fmaxf(v[e], 0.f);
        }
        const uint4 pk = O::store_vals(v);
        if constexpr (E == 4) {
          *reinterpret_cast<uint4*>(yp + pix + co) = pk;
        } else {
          *reinterpret_cast<uint2*>(yp + pix + co) = make_uint2(pk.x, pk.y);
        }
      }
    }
  } else {
    // ---- epilogue through LDS, PR rows per pass: the accumulators (BN applied) are
    // staged as an f32 [pixel][channel] tile, then written as whole 16-B NHWC chunks
    // with residual add + ReLU (mode 0), as NCHW f32 planes (mode 1), as f32 GEMM rows (mode 2)
    // or fed to the fused 1x1 head (g.hm, single pass)
    float* Cs = reinterpret_cast<float*>(smem);
    constexpr int CPR = BN / E;            // output chunks per tile row
    constexpr int ITER = PR * CPR / NT;    // chunks per thread per pass
    static_assert(ITER * NT == PR * CPR, "epilogue chunk split");
    const bool mode0 = !SPL && g.mode == 0 && !g.hm;  // (split NHWC outputs take the direct epilogue)
    const bool relu_at_stage = g.relu && !mode0;  // mode 0: ReLU after the residual add
    const int HoWo = om.HoWo;
    float sc[TN][4], sh[TN][4];
    params4(sc, sh);
#pragma unroll
    for (int p = 0; p < BM / PR; ++p) {
      // residual chunks of this pass first (their latency overlaps the staging)
      const T* __restrict__ rp = reinterpret_cast<const T*>(g.res);
      size_t off[ITER];
      bool ok[ITER];
      uint4 rv[ITER];
      if (mode0) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
          const int idx = tid + it * NT;
          const int row = idx / CPR, cc = idx - row * CPR;
          const int m = m0 + p * PR + row, co = n0 + cc * E;
          ok[it] = m < g.M && co < g.Cout;
          off[it] = om.nhwc(ok[it] ? m : 0, g.Cout) + (ok[it] ? co : 0);
          rv[it] = make_uint4(0, 0, 0, 0);
          if (rp && ok[it]) rv[it] = *reinterpret_cast<const uint4*>(rp + off[it]);
        }
      }
      __syncthreads();  // the ring (or the previous pass) is no longer read
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = rowA(i) + r16 - p * PR;
        if (rowA(i) / PR != p) continue;  // wave-uniform
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int colb = colB(j) + q * 4;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = acc[i][j][e] * sc[j][e] + sh[j][e];
            if (relu_at_stage) v[e] = fmaxf(v[e], 0.f);
          }
          *reinterpret_cast<float4*>(Cs + row * LD + colb) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
      __syncthreads();
      if (mode0) {
        T* __restrict__ yp = reinterpret_cast<T*>(g.y);
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
          if (!ok[it]) continue;
          const int idx = tid + it * NT;
          const int row = idx / CPR, cc = idx - row * CPR;
          float v[E];
          staged_vals(Cs, row, cc, v);
          if (rp) {
            float r[E];
            O::load_vals(rv[it], r);
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] += r[e];
          }
          if (g.relu) {
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = fmaxf(v[e], 0.f);
          }
          *reinterpret_cast<uint4*>(yp + off[it]) = O::store_vals(v);
        }
      } else if (g.mode == 2) {
        // f32 GEMM rows, column blocks of vblk stored as separate [M][vblk] planes
        float* __restrict__ yp = reinterpret_cast<float*>(g.y);
        for (int idx = tid; idx < PR * CPR; idx += NT) {
          const int row = idx / CPR, cc = idx - row * CPR;
          const int m = m0 + p * PR + row, co = n0 + cc * E;
          if (m >= g.M || co >= g.Cout) continue;
          const int blk = co / g.vblk, cin = co - blk * g.vblk;
          float* dst = yp + (static_cast<size_t>(blk) * g.M + m) * g.vblk + cin;
#pragma unroll
          for (int e = 0; e < E; e += 4)
            *reinterpret_cast<float4*>(dst + e) = *reinterpret_cast<const float4*>(Cs + row * LD + cc * E + e);
        }
      } else if (!g.hm) {
        // NCHW f32 (heatmap head): consecutive threads walk pixels of one channel
        float* __restrict__ yp = reinterpret_cast<float*>(g.y);
        const int ncol = min(BN, g.Cout - n0);
        for (int idx = tid; idx < PR * ncol; idx += NT) {
          const int col = idx / PR, row = idx - col * PR;
          const int m = m0 + p * PR + row;
          if (m >= g.M) continue;
          const int n = m / HoWo, pixo = m - n * HoWo;
          yp[(static_cast<size_t>(n) * g.Cout + n0 + col) * HoWo + pixo] = Cs[row * LD + col];
        }
      } else if constexpr (!SPL && BN == 256 && BM == 64 && PR == BM && NW == 4) {
      // the f32 fused head: one 64x256 block owns all 256 output channels of its pixels, staged in Cs
        constexpr int CPR = BN / E;
        // optional store of the deconv output f (NHWC), values rounded to T in place so
        // the head sees exactly what a separate head launch would read
        T* __restrict__ yp = reinterpret_cast<T*>(g.y);
        for (int idx = tid; idx < BM * CPR; idx += NT) {
          const int row = idx / CPR, cc = idx - row * CPR;
          const int m = m0 + row;
          float v[E];
          staged_vals(Cs, row, cc, v);
          const uint4 packed = O::store_vals(v);
          float vr[E];
          O::load_vals(packed, vr);
    #pragma unroll
          for (int e = 0; e < E; e += 4)
            *reinterpret_cast<float4*>(Cs + row * LD + cc * E + e) = make_float4(vr[e], vr[e + 1], vr[e + 2], vr[e + 3]);
          if (yp && m < g.M) *reinterpret_cast<uint4*>(yp + om.nhwc(m, g.Cout) + cc * E) = packed;
        }
        __syncthreads();
        // final_layer (pose_resnet.py:126-132, 203) on the tile in LDS: wave w takes
        // pixel rows 16w..16w+15, one 16x16 MFMA tile = 16 joints, K = Cout
        f32x4 hacc = f32x4{0.f, 0.f, 0.f, 0.f};
        const T* __restrict__ hwp = reinterpret_cast<const T*>(g.hw);
        const int hrow = wid * 16 + r16;
        for (int kc = 0; kc < g.Cout / (4 * E); ++kc) {
          const int c = 4 * kc + q;
          float av[E];
          staged_vals(Cs, hrow, c, av);
          const uint4 a = O::store_vals(av);
          const uint4 b = *reinterpret_cast<const uint4*>(hwp + static_cast<size_t>(r16) * g.hkp + c * E);
          O::mma(hacc, a, b);  // rows = pixels, cols = joints
        }
        const int joint = r16;
        if (joint < g.J) {
          const float bj = g.hbias ? g.hbias[joint] : 0.f;
          const int HWo = g.out_H * g.out_W;
    #pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int m = m0 + wid * 16 + q * 4 + e;
            if (m < g.M) {
              int n;
              const int pixo = om.plane(m, n);
              g.hm[(static_cast<size_t>(n) * g.J + joint) * HWo + pixo] = hacc[e] + bj;
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// Persistent variant (2-byte dtypes, direct NHWC epilogue).  The grid is the resident
// block count; each block walks a run of tiles (every XCD owns a contiguous slice of the
// tile order, so its concurrently running tiles still share operand rows in its L2) as ONE
// flattened stream of K-tiles through an S-slot LDS-DMA ring: the DMA of the next tile's
// first K-tiles is already in flight while the current tile's epilogue stores drain, and
// the stores never block the stream -- every epilogue issues exactly NST buffer stores per
// thread (out-of-range rows go to an offset past num_records), so each wait is a counted
// vmcnt that retires the K-tile being consumed and nothing younger.
template <typename T, int BM, int BN, int NW, int WGM, int S, bool DUAL>
__global__ __launch_bounds__(NW * 64) void conv_persist_kernel(ConvGeom g) {
  using C = TileCfg<T, BM, BN, NW, WGM, S, DUAL>;
  using O = Op<T>;
  constexpr int E = C::E, ES = C::ES, BK = C::BK;
  constexpr int WTM = C::WTM, WTN = C::WTN, TM = C::TM, TN = C::TN;
  constexpr int RA = C::RA, ND = C::ND, A_BYTES = C::A_BYTES, STAGE = C::STAGE;
  constexpr int TP = TN / 2;
  constexpr int NST = TM * TP;  // 16-B stores per thread per tile
  static_assert(E == 8 && TN % 2 == 0, "persistent variant: 2-byte dtypes, paired n-tiles");
  static_assert(S == 2 || S == 3, "2 or 3 ring slots");
  static_assert(ND * (S - 2) + 2 * NST < 64, "vmcnt range");
  __shared__ __attribute__((aligned(16))) char smem[ring_bytes<BM, BN, S>()];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wm = wid / C::WGN, wn = wid % C::WGN;
  const int r16 = lane & 15, q = lane >> 4;

  // ---- this block's tiles: XCD xcd = blockIdx & 7 owns tiles [cstart, cstart + clen);
  // its nslot blocks take them round robin
  const int ntile = g.mtiles * g.ntiles * (g.deconv ? 4 : 1);
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
  const int qq = ntile >> 3, rr = ntile & 7;
  const int cstart = xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq;
  const int clen = qq + (xcd < rr ? 1 : 0);
  const int ntl = slot < clen ? (clen - slot + nslot - 1) / nslot : 0;
  const int nk = g.Kpad / BK;
  const int total = ntl * nk;
  if (total == 0) return;

  auto decode = [&](int k, int& mt, int& cls, int& nt) {
    const int w = cstart + slot + k * nslot;
    nt = w % g.ntiles;
    const int rest = w / g.ntiles;
    mt = g.deconv ? rest >> 2 : rest;
    cls = g.deconv ? rest & 3 : 0;
  };

  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) char*)smem));
  const unsigned wid_u = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(wid));

  // ---- load side: geometry of the tile whose K-tiles the DMA is fetching
  int l_tile = -1;
  Gather<C> ga;
  ga.init(g, tid);
  // DMA of stream K-tile sq into ring slot sq % S: exactly ND dma16 per thread.  The
  // source offsets are computed first (dma_prep), the instructions issued by dma_issue(d)
  // -- all at once, or (eight-wave tiles) interleaved with the previous K-tile's MFMAs.
  int doff[ND];
  unsigned dAs = 0;
  bool dsec = false;
  auto dma_prep = [&](int sq) {
    const int k = sq / nk, kt = sq - k * nk;
    if (k != l_tile) {
      int mt, cls, nt;
      decode(k, mt, cls, nt);
      ga.set_tile(g, tid, mt * BM, nt * BN, class_geom(g, cls));
      l_tile = k;
    }
    dAs = __builtin_amdgcn_readfirstlane(lds0 + (sq % S) * STAGE + wid_u * 1024);
    if constexpr (DUAL) dsec = __builtin_amdgcn_readfirstlane(ga.second(g, kt) ? 1 : 0) != 0;
    ga.a_offsets(g, kt, [&](int i, int off) { doff[i] = off; });
    ga.b_offsets(g, kt, [&](int i, int off) { doff[RA + i] = off; });
  };
  auto dma_issue = [&](int d) {  // d compile-time after unrolling
    if (d < RA) {
      if (DUAL && dsec) dma16(ga.x2rs, doff[d], dAs + d * NW * 1024);
      else dma16(ga.xrs, doff[d], dAs + d * NW * 1024);
    } else {
      dma16(ga.wrs, doff[d], dAs + A_BYTES + (d - RA) * NW * 1024);
    }
  };
  auto dma_ktile = [&](int sq) {
    dma_prep(sq);
#pragma unroll
    for (int d = 0; d < ND; ++d) dma_issue(d);
  };
  constexpr bool IL = NW == 8;  // interleave the next K-tile's DMAs with the MFMAs
  constexpr int IL_STEP = 4;    // one DMA after every IL_STEP MFMAs
  static_assert(!IL || ND * IL_STEP <= 2 * TM * TN, "interleave slots");

  f32x4 acc[TM][TN];
  auto zero_acc = [&] {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto compute = [&](int slot_, bool more) {
    mma_ktile<C>(smem + slot_ * STAGE, wm * WTM + r16, wn * WTN + r16, q, acc, [&](int f) {
      if constexpr (IL) {
        if (f % IL_STEP == IL_STEP - 1 && f / IL_STEP < ND && more) {
          __builtin_amdgcn_sched_barrier(0);
          dma_issue(f / IL_STEP);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    });
  };
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
      g.y, 0, g.N * g.out_H * g.out_W * g.Cout * ES, 0x00020000);
  const T* __restrict__ rp = reinterpret_cast<const T*>(g.res);
  // Small tiles load the residual with counted (inline-asm) loads issued before the last
  // K-tile's wait, so the epilogue waits only for them -- not for the DMA issued after.
  constexpr bool ARES = TM * TP <= 8;
  constexpr int NR = ARES ? TM * TP : 0;
  const u32x4 rrs = make_srd(g.res ? g.res : g.y, g.N * g.out_H * g.out_W * g.Cout * ES);
  u32x4 rres[ARES ? TM : 1][ARES ? TP : 1];
  // store side of stream tile k: its rows' output pixels (element offsets, row 0 where m is past M)
  // and the first of this lane's 8 channels of pair jp
  auto out_rows = [&](int k, int& n0, OutMap& om) {
    int mt, cls, nt;
    decode(k, mt, cls, nt);
    n0 = nt * BN;
    om = class_geom(g, cls).out;
    return mt * BM;
  };
  auto out_pix = [&](const OutMap& om, int m0, int i, bool& mok) {
    const int m = m0 + wm * WTM + i * 16 + r16;
    mok = m < g.M;
    return om.nhwc<int>(mok ? m : 0, g.Cout);
  };
  auto pair_ch = [&](int n0, int jp) { return n0 + wn * WTN + (2 * jp + (q & 1)) * 16 + 8 * (q >> 1); };
  auto res_issue = [&](int k) {
    int n0;
    OutMap om;
    const int m0 = out_rows(k, n0, om);
    asm volatile("s_nop 4" ::: "memory");
#pragma unroll
    for (int i = 0; i < (ARES ? TM : 1); ++i) {
      bool mok;
      const int pix = out_pix(om, m0, i, mok);
#pragma unroll
      for (int jp = 0; jp < (ARES ? TP : 1); ++jp) {
        const int co = pair_ch(n0, jp);
        const int off = (mok && co < g.Cout) ? (pix + co) * ES : kOOB;
        asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(rres[i][jp]) : "v"(off), "s"(rrs) : "memory");
      }
    }
  };
  const bool ares = ARES && g.res != nullptr;
  // epilogue of stream tile k: BN, residual, ReLU in registers; NST 16-B buffer stores
  auto epilogue = [&](int k) {
    int n0;
    OutMap om;
    const int m0 = out_rows(k, n0, om);
    int cop[TP];
    float sc[TP][8], sh[TP][8];
#pragma unroll
    for (int jp = 0; jp < TP; ++jp) {
      cop[jp] = pair_ch(n0, jp);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int co = cop[jp] + e;
        sc[jp][e] = (co < g.Cout && g.scale) ? g.scale[co] : 1.f;
        sh[jp][e] = (co < g.Cout && g.shift) ? g.shift[co] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      bool mok;
      const int pix = out_pix(om, m0, i, mok);
      uint4 rv[TP];
#pragma unroll
      for (int jp = 0; jp < TP; ++jp) {
        rv[jp] = make_uint4(0, 0, 0, 0);
        if constexpr (ARES) {
          if (ares) {
            rv[jp] = make_uint4(rres[i][jp].x, rres[i][jp].y, rres[i][jp].z, rres[i][jp].w);
            continue;
          }
        }
        if (rp && mok && cop[jp] < g.Cout) rv[jp] = *reinterpret_cast<const uint4*>(rp + pix + cop[jp]);
      }
#pragma unroll
      for (int jp = 0; jp < TP; ++jp) {
        float v[8], r[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][2 * jp][e]),
                                                           __float_as_uint(acc[i][2 * jp + 1][e]), false, false);
          v[e] = __uint_as_float(sw[0]);
          v[4 + e] = __uint_as_float(sw[1]);
        }
        O::load_vals(rv[jp], r);
        affine8<false>(v, sc[jp], sh[jp]);
        if (rp) add8<false>(v, r);
        if (g.relu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        const uint4 pk = O::store_vals(v);
        const u32x4 pv = {pk.x, pk.y, pk.z, pk.w};
        const int voff = (mok && cop[jp] < g.Cout) ? (pix + cop[jp]) * ES : kOOB;
        __builtin_amdgcn_raw_buffer_store_b128(pv, yrs, voff, 0, 0);
      }
    }
  };
  auto barrier = [] {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  zero_acc();
  unsigned wv[kWarmLoads];   // weight warm-up (gemm_common.h), consumed after the first DMAs
  warm_issue(wv, g.w, g.wseg, g.warm, NW * 64);
#pragma unroll
  for (int sq = 0; sq < S - 1; ++sq)
    if (sq < total) dma_ktile(sq);
  warm_use(wv);
  for (int sq = 0; sq < total; ++sq) {
    const bool tile_end = (sq + 1) % nk == 0;
    if (ares && tile_end) res_issue(sq / nk);
    // retire K-tile sq: younger = the DMA groups of sq+1 .. sq+S-2, the stores of the
    // epilogues run since sq's DMA was issued (iterations sq-S+1 .. sq-1) and the
    // residual loads just issued
    const int a = min(S - 2, total - 1 - sq);
    int e = 0;
#pragma unroll
    for (int d = 1; d < S; ++d) e += (sq - d >= 0 && (sq - d + 1) % nk == 0) ? 1 : 0;
    vm_wait_dyn(ND * a + NST * e + ((ares && tile_end) ? NR : 0));
    barrier();
    const bool more = sq + S - 1 < total;
    if (IL) {
      if (more) dma_prep(sq + S - 1);
    } else if (more) {
      dma_ktile(sq + S - 1);
    }
    compute(sq % S, more);
    if (tile_end) {
      if constexpr (ARES) {
        if (ares) {  // the residual has landed once only this iteration's DMA group is younger
          if (more) vm_wait<ND>();
          else vm_wait<0>();
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int jp = 0; jp < TP; ++jp) asm volatile("" : "+v"(rres[i][jp]));
        }
      }
      epilogue(sq / nk);
      zero_acc();
    }
  }
}

}  // namespace
}  // namespace posu
