// Heatmap mutual-information loss: the pair scores of HeatmapDiscriminator over all Q x Q
// (feature row, heatmap value) pairs of every image (reference lib/core/loss.py:674-717 +
// lib/models/discriminator.py:225-242), their backward, and the JSD / InfoNCE measures on the
// scores (loss.py:719-757).
//
// The reference materialises the pairs as a dense [N Q Q, C + 1] tensor.  Here nothing per pair is
// stored except the score: Linear(C + 1 -> cm, no bias) over the concatenation [h | f] splits into
//     z1[n, i, j, :] = A[n, i, :] + h[n, j] * w_h,   A = F_s W_f^T  ([N, Q, cm]),  W1 = [w_h | W_f],
// so a pass over the pairs holds one A row per lane, reads one heatmap value per pair and recomputes
// BN1 -> LeakyReLU -> Linear(cm -> cm/4) -> BN2 -> LeakyReLU -> Linear(cm/4 -> 1) in registers.
// BN1's batch statistics are a closed form in the per-image sums of A, A^2, h and h^2; BN2's need
// a pass of their own.  Passes (every one over all pairs, lane = row (n, i), waves and grid.z over j):
//     forward   k_stats  sum z2, sum z2^2            -> BN2 mean / variance
//               k_score  u
//     backward  k_b1     sum dy2, sum dy2 xhat2, sum du a2, sum du          -> d gamma2, d beta2, d w3, d b3
//               k_b2     dz2 -> d b2, d W2 (via an LDS tile), sum dy1, sum dy1 xhat1 -> d gamma1, d beta1
//               k_b3     dz1 -> dA (summed over j in the lane), t = dz1 . w_h per pair, d w_h
//     then dh = sum_i t, d W_f = dA^T F_s, and the scatter of dA W_f / dh to the sampled positions
//     (a repeated position takes the sum over its occurrences, added in index order).
//
// Reductions follow bn_train.hip: f64 partials per block (per wave for the LDS-tile sums) in the
// caller's workspace, summed in a fixed order by a finalise kernel; no floating-point atomics, so
// two runs give the same bits.  Arithmetic is f32; sums that cross pairs are f64.
#include <type_traits>

#include "posu_common.h"

namespace posu {
namespace {

constexpr int kMaxNB = 32;      // blocks per (segment, j slab): bounds the partial count
constexpr int kMaxJS = 4;        // j slabs (grid.z) of the passes that keep nothing per row
constexpr float kSlope = 0.2f;   // LeakyReLU(0.2)
constexpr int kGatherRows = 8;   // rows per block of the A = F_s W_f^T kernel
constexpr int kMiNB = 64;        // blocks per segment of the measure's forward

// indices into the host array of parameter pointers (include/posu.h)
enum Param { P_W1, P_G1, P_BE1, P_RM1, P_RV1, P_W2, P_B2, P_G2, P_BE2, P_RM2, P_RV2, P_W3, P_B3, P_COUNT };

// threads per block of the pair passes: the cm = 128 net holds twice the registers per lane
template <int CM>
constexpr int pair_threads() { return CM == 128 ? 128 : 256; }

// Doubles per partial of each pair pass, P = (seg * JS + z) * NBx + bx the block's index:
//   stats  part[P][2 K2]          sum z2 | sum z2^2
//   b1     part[P][3 K2 + 1]      sum dy2 | sum dy2 xhat2 | sum du a2 | sum du
//   b2     part[P][K2]            sum dz2                                          (per block)
//   b2w    wpart[P * NW + w][K2 cm + 2 cm]   d W2 | sum dy1 | sum dy1 xhat1         (per wave)
//   b3     part[P][cm]            sum dz1 h
struct PartLen {
  int stats, b1, b2, b2w, b3;
};
constexpr PartLen part_len(int cm) { return {2 * (cm / 4), 3 * (cm / 4) + 1, cm / 4, (cm / 4) * cm + 2 * cm, cm}; }

// Per-segment derived values (f32), written by the finalisers between the passes: six arrays per
// BatchNorm (scale, shift, mean, 1 / std, and the two means its backward subtracts), cm wide for
// BN1 and K2 wide for BN2.
enum DrvSlot { D_SC, D_SH, D_MEAN, D_RSTD, D_MA, D_MB, D_SLOTS };
constexpr int drv_stride(int cm) { return D_SLOTS * (cm + cm / 4); }
template <int CM>
struct Drv {
  static constexpr int K2 = CM / 4, STRIDE = drv_stride(CM);
  const float *sc1, *sh1, *mean1, *rstd1, *m1a, *m1b, *sc2, *sh2, *mean2, *rstd2, *m2a, *m2b;
  // array `slot` of BN1 (cm wide) / BN2 (K2 wide) of segment seg
  template <typename F>
  __device__ __forceinline__ static F* bn1(F* drv, int seg, int slot) {
    return drv + static_cast<size_t>(seg) * STRIDE + slot * CM;
  }
  template <typename F>
  __device__ __forceinline__ static F* bn2(F* drv, int seg, int slot) {
    return drv + static_cast<size_t>(seg) * STRIDE + D_SLOTS * CM + slot * K2;
  }
  __device__ __forceinline__ Drv(const float* d, int seg) {
    sc1 = bn1(d, seg, D_SC), sh1 = bn1(d, seg, D_SH), mean1 = bn1(d, seg, D_MEAN), rstd1 = bn1(d, seg, D_RSTD);
    m1a = bn1(d, seg, D_MA), m1b = bn1(d, seg, D_MB);
    sc2 = bn2(d, seg, D_SC), sh2 = bn2(d, seg, D_SH), mean2 = bn2(d, seg, D_MEAN), rstd2 = bn2(d, seg, D_RSTD);
    m2a = bn2(d, seg, D_MA), m2b = bn2(d, seg, D_MB);
  }
};

// The batch statistics handed back to the caller, stats[seg][3][cm + K2]: mean, biased and unbiased
// variance; BN1's cm columns, then BN2's K2.
template <int CM>
__device__ __forceinline__ float& stat_at(float* stats, int seg, int which, int col) {
  return stats[(static_cast<size_t>(seg) * 3 + which) * (CM + CM / 4) + col];
}

// One channel of a BatchNorm: mean and variance from the sums over the M rows (training; also into
// column `col` of the stats) or from the running statistics, then the six derived values, `d` the
// channel's entry of the layer's first array (slot D_SC) and W the arrays' width.
template <int CM>
__device__ __forceinline__ void bn_finish(int training, double a1, double a2, double M, const float* rm,
                                          const float* rv, const float* gamma, const float* beta, int i, float eps,
                                          float* stats, int seg, int col, float* d, int W) {
  double mean, var;
  if (training) {
    mean = a1 / M;
    var = a2 / M - mean * mean;
    if (var < 0.0) var = 0.0;
    stat_at<CM>(stats, seg, 0, col) = static_cast<float>(mean);
    stat_at<CM>(stats, seg, 1, col) = static_cast<float>(var);
    stat_at<CM>(stats, seg, 2, col) = static_cast<float>(var * (M / (M - 1.0)));
  } else {
    mean = rm[i];
    var = rv[i];
  }
  const double rstd = 1.0 / sqrt(var + static_cast<double>(eps));
  const double sc = gamma[i] * rstd;
  d[D_SC * W] = static_cast<float>(sc);
  d[D_SH * W] = static_cast<float>(beta[i] - mean * sc);
  d[D_MEAN * W] = static_cast<float>(mean);
  d[D_RSTD * W] = static_cast<float>(rstd);
  d[D_MA * W] = 0.f;
  d[D_MB * W] = 0.f;
}

template <typename T>
__device__ __forceinline__ float ldf(const T* p, size_t i);
template <>
__device__ __forceinline__ float ldf<float>(const float* p, size_t i) { return p[i]; }
template <>
__device__ __forceinline__ float ldf<uint16_t>(const uint16_t* p, size_t i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float ldf<f16_t>(const f16_t* p, size_t i) {
  return static_cast<float>(__builtin_bit_cast(_Float16, p[i].bits));
}
__device__ __forceinline__ void stf(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void stf(uint16_t* p, size_t i, float v) { p[i] = f2bf(v); }
__device__ __forceinline__ void stf(f16_t* p, size_t i, float v) {
  p[i].bits = __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
}

__device__ __forceinline__ float leaky(float y) { return y > 0.f ? y : kSlope * y; }
__device__ __forceinline__ float leaky_slope(float y) { return y > 0.f ? 1.f : kSlope; }
// The sampled position of row (g, i), clamped to the map: an index outside it is the caller's
// contract (refused on the host when it hands a host copy), never an access outside.
__device__ __forceinline__ int sample_pos(const int* idx, int row, int HW) {
  const int v = idx[row];
  return v < 0 ? 0 : (v > HW - 1 ? HW - 1 : v);
}

// Sum of every thread's acc[q] in a fixed order (a tree over the thread index), written by thread 0
template <int NACC>
__device__ __forceinline__ void block_reduce_store(const double* acc, double* out) {
  __shared__ double red[256];
  const int tid = threadIdx.x, nt = blockDim.x;
#pragma unroll
  for (int q = 0; q < NACC; ++q) {
    red[tid] = acc[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s && tid + s < nt) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) out[q] = red[0];
    __syncthreads();
  }
}

// ------------------------------------------------------------------ A = F_s W_f^T, h, w_h
// One block per kGatherRows rows (g, i): the gathered feature rows staged in LDS as f32, thread
// (c, row group) sums over the C channels.
template <typename T, int CM>
__global__ __launch_bounds__(256) void k_gather(const T* __restrict__ feat, const float* __restrict__ hm,
                                                const int* __restrict__ idx, const float* __restrict__ W1,
                                                int rows, int Q, int HW, int C, int J, int joint,
                                                float* __restrict__ A, float* __restrict__ h,
                                                float* __restrict__ wh) {
  __shared__ float fs[kGatherRows][512];
  const int tid = threadIdx.x, r0 = blockIdx.x * kGatherRows, ldw = C + 1;
  for (int e = tid; e < kGatherRows * C; e += 256) {
    const int r = e / C, ch = e - r * C, row = r0 + r;
    float v = 0.f;
    if (row < rows) {
      const int g = row / Q, pos = sample_pos(idx, row, HW);
      v = ldf<T>(feat, (static_cast<size_t>(g) * HW + pos) * C + ch);
    }
    fs[r][ch] = v;
  }
  if (tid < kGatherRows && r0 + tid < rows) {
    const int row = r0 + tid, g = row / Q, pos = sample_pos(idx, row, HW);
    h[row] = hm[(static_cast<size_t>(g) * J + joint) * HW + pos];
  }
  if (blockIdx.x == 0 && tid < CM) wh[tid] = W1[static_cast<size_t>(tid) * ldw];
  __syncthreads();
  constexpr int NG = 256 / CM, RPT = (kGatherRows + NG - 1) / NG;
  const int c = tid % CM, rg = tid / CM;
  float acc[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) acc[k] = 0.f;
  const float* w = W1 + static_cast<size_t>(c) * ldw + 1;
  for (int ch = 0; ch < C; ++ch) {
    const float wv = w[ch];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int r = rg + k * NG;
      if (r < kGatherRows) acc[k] = __builtin_fmaf(fs[r][ch], wv, acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int r = rg + k * NG, row = r0 + r;
    if (r < kGatherRows && row < rows) A[static_cast<size_t>(row) * CM + c] = acc[k];
  }
}

// ------------------------------------------------------------------ BN1 statistics, closed form
// Over a segment's N Q^2 rows z1 = A[n, i] + h[n, j] w_h:
//   sum z1   = sum_n ( Q SA_n + Q w_h Sh_n )
//   sum z1^2 = sum_n ( Q SAA_n + 2 w_h SA_n Sh_n + Q w_h^2 Shh_n )
// with the per-image sums over i (A) and j (h), all in f64.  One block per segment; thread (c, part)
// takes the images n = part mod NP, the parts are added in order.  training == 0: the running
// statistics instead.
template <int CM>
__global__ __launch_bounds__(256) void k_bn1(const float* __restrict__ A, const float* __restrict__ h,
                                             const float* __restrict__ wh, const float* __restrict__ g1,
                                             const float* __restrict__ be1, const float* __restrict__ rm1,
                                             const float* __restrict__ rv1, int N, int Q, int training, float eps,
                                             float* __restrict__ drv, float* __restrict__ stats) {
  constexpr int NP = 256 / CM;
  __shared__ double s1[NP][CM], s2[NP][CM];
  const int seg = blockIdx.x, tid = threadIdx.x, c = tid % CM, part = tid / CM;
  if (training) {
    const double w = wh[c];
    double a1 = 0.0, a2 = 0.0;
    for (int n = part; n < N; n += NP) {
      const size_t r0 = (static_cast<size_t>(seg) * N + n) * Q;
      double sa = 0.0, saa = 0.0, sh = 0.0, shh = 0.0;
      for (int i = 0; i < Q; ++i) {
        const double a = A[(r0 + i) * CM + c], hv = h[r0 + i];
        sa += a;
        saa += a * a;
        sh += hv;
        shh += hv * hv;
      }
      a1 += Q * sa + Q * w * sh;
      a2 += Q * saa + 2.0 * w * sa * sh + Q * w * w * shh;
    }
    s1[part][c] = a1;
    s2[part][c] = a2;
  }
  __syncthreads();
  if (part != 0) return;
  double a1 = 0.0, a2 = 0.0;
  if (training) {
    for (int p = 0; p < NP; ++p) {
      a1 += s1[p][c];
      a2 += s2[p][c];
    }
  }
  bn_finish<CM>(training, a1, a2, static_cast<double>(N) * Q * Q, rm1, rv1, g1, be1, c, eps, stats, seg, c,
                Drv<CM>::bn1(drv, seg, D_SC) + c, CM);
}

// ------------------------------------------------------------------ the pair passes
// What the five passes share.  The walk: block (bx, seg, z) takes the chunks bx, bx + NBx, .. of 64
// rows of its segment (lane = row) and the j slab z of Q; wave w of its NW takes j = jlo + w,
// jlo + w + NW, ..  A lane past the last row, and a wave past the slab's last j, computes on the
// clamped row / j and contributes nothing (`valid`, `act`), so every barrier is met by all.
template <int CM>
struct Walk {
  static constexpr int NT = pair_threads<CM>(), NW = NT / 64;
  int seg, Q, NQ, nch, tid, lane, wave, jlo, jhi, niter;
  __device__ __forceinline__ Walk(int N, int Q_) {
    seg = blockIdx.y, Q = Q_, NQ = N * Q, nch = (NQ + 63) / 64;
    tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int JS = gridDim.z;
    jlo = static_cast<int>(static_cast<long long>(Q) * blockIdx.z / JS);
    jhi = static_cast<int>(static_cast<long long>(Q) * (blockIdx.z + 1) / JS);
    niter = (jhi - jlo + NW - 1) / NW;
  }
  __device__ __forceinline__ size_t partial() const {  // the block's partial index P
    return (static_cast<size_t>(seg) * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x;
  }
  struct Chunk {
    int grow, g;  // global row (g, i) of the lane, clamped; g = grow / Q
    bool valid;
  };
  __device__ __forceinline__ Chunk chunk(int ch) const {
    const int row = ch * 64 + lane;
    const bool valid = row < NQ;
    const int grow = seg * NQ + (valid ? row : NQ - 1);
    return {grow, grow / Q, valid};
  }
  struct Step {
    int jc, pair;  // clamped j; index of (grow, jc) in u, du and t
    bool act;
  };
  __device__ __forceinline__ Step step(const Chunk& r, int it) const {
    const int j = jlo + it * NW + wave, jc = j < jhi ? j : jhi - 1;
    return {jc, r.grow * Q + jc, r.valid && j < jhi};
  }
};

template <int CM>
__device__ __forceinline__ void load_row(const float* Arow, float* a) {
#pragma unroll
  for (int c4 = 0; c4 < CM / 4; ++c4) {
    const float4 v = *reinterpret_cast<const float4*>(Arow + 4 * c4);
    a[4 * c4] = v.x, a[4 * c4 + 1] = v.y, a[4 * c4 + 2] = v.z, a[4 * c4 + 3] = v.w;
  }
}

// Channel c of one pair up to BN1's output.  The two loops over W2 that follow it in a pass (a1 into z2, dz2
// into da1) stay in the kernels, in the same nesting and statement order in each: one helper around
// them, whether it takes z2 through a pointer or returns it in a struct, is unrolled on its own before it
// is inlined, fewer of the W2 loads are paired afterwards, and k_score<64> went from 109 to 143 us
// (profiles/r08/heatmap_mi_refactor_micro.txt, with the scratch each form costs at c_m = 128).
struct Fwd1 {
  float z1, y1;
};
template <int CM>
__device__ __forceinline__ Fwd1 fwd1(float h, float a, int c, const float* wh, const Drv<CM>& v) {
  const float z1 = __builtin_fmaf(h, wh[c], a);
  return {z1, __builtin_fmaf(z1, v.sc1[c], v.sh1[c])};
}
template <int CM>
__device__ __forceinline__ float act1(float h, float a, int c, const float* wh, const Drv<CM>& v) {
  return leaky(fwd1<CM>(h, a, c, wh, v).y1);
}

// Backward through Linear3, LeakyReLU and BN2 at output k of one pair
struct Back2 {
  float y2, xh2, dy2, dz2;
};
template <int CM>
__device__ __forceinline__ Back2 back2(float z2, float duv, bool act, int k, const float* w3,
                                       const Drv<CM>& v) {
  Back2 b;
  b.y2 = __builtin_fmaf(z2, v.sc2[k], v.sh2[k]);
  b.xh2 = (z2 - v.mean2[k]) * v.rstd2[k];
  b.dy2 = duv * w3[k] * leaky_slope(b.y2);
  b.dz2 = act ? v.sc2[k] * (b.dy2 - v.m2a[k] - b.xh2 * v.m2b[k]) : 0.f;
  return b;
}

template <int CM>
__global__ __launch_bounds__(pair_threads<CM>()) void k_stats(
    const float* __restrict__ A, const float* __restrict__ hbuf, const float* __restrict__ wh,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ drv,
    double* __restrict__ part, int N, int Q) {
  constexpr int K2 = CM / 4, L = part_len(CM).stats;
  const Walk<CM> w(N, Q);
  const Drv<CM> v(drv, w.seg);
  double acc[L];
#pragma unroll
  for (int q = 0; q < L; ++q) acc[q] = 0.0;
  for (int ch = blockIdx.x; ch < w.nch; ch += gridDim.x) {
    const auto r = w.chunk(ch);
    float Areg[CM];
    load_row<CM>(A + static_cast<size_t>(r.grow) * CM, Areg);
    for (int it = 0; it < w.niter; ++it) {
      const auto s = w.step(r, it);
      const float h = hbuf[r.g * Q + s.jc];
      float z2[K2];
#pragma unroll
      for (int k = 0; k < K2; ++k) z2[k] = b2[k];
#pragma unroll
      for (int c4 = 0; c4 < CM / 4; ++c4) {
        float a4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a4[e] = Areg[4 * c4 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a1 = act1<CM>(h, a4[e], 4 * c4 + e, wh, v);
#pragma unroll
          for (int k = 0; k < K2; ++k) z2[k] = __builtin_fmaf(W2[k * CM + 4 * c4 + e], a1, z2[k]);
        }
      }
      if (s.act) {
#pragma unroll
        for (int k = 0; k < K2; ++k) {
          const double z = z2[k];
          acc[k] += z;
          acc[K2 + k] += z * z;
        }
      }
    }
  }
  block_reduce_store<L>(acc, part + w.partial() * L);
}

template <int CM>
__global__ __launch_bounds__(pair_threads<CM>()) void k_score(
    const float* __restrict__ A, const float* __restrict__ hbuf, const float* __restrict__ wh,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, const float* __restrict__ drv, float* __restrict__ u, int N, int Q) {
  constexpr int K2 = CM / 4;
  const Walk<CM> w(N, Q);
  const Drv<CM> v(drv, w.seg);
  for (int ch = blockIdx.x; ch < w.nch; ch += gridDim.x) {
    const auto r = w.chunk(ch);
    float Areg[CM];
    load_row<CM>(A + static_cast<size_t>(r.grow) * CM, Areg);
    for (int it = 0; it < w.niter; ++it) {
      const auto s = w.step(r, it);
      const float h = hbuf[r.g * Q + s.jc];
      float z2[K2];
#pragma unroll
      for (int k = 0; k < K2; ++k) z2[k] = b2[k];
#pragma unroll
      for (int c4 = 0; c4 < CM / 4; ++c4) {
        float a4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a4[e] = Areg[4 * c4 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a1 = act1<CM>(h, a4[e], 4 * c4 + e, wh, v);
#pragma unroll
          for (int k = 0; k < K2; ++k) z2[k] = __builtin_fmaf(W2[k * CM + 4 * c4 + e], a1, z2[k]);
        }
      }
      float sc = b3[0];
#pragma unroll
      for (int k = 0; k < K2; ++k) sc = __builtin_fmaf(w3[k], leaky(__builtin_fmaf(z2[k], v.sc2[k], v.sh2[k])), sc);
      if (s.act) u[s.pair] = sc;
    }
  }
}

template <int CM>
__global__ __launch_bounds__(pair_threads<CM>()) void k_b1(
    const float* __restrict__ A, const float* __restrict__ hbuf, const float* __restrict__ wh,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ drv, const float* __restrict__ du, double* __restrict__ part, int N, int Q) {
  constexpr int K2 = CM / 4, L = part_len(CM).b1;
  const Walk<CM> w(N, Q);
  const Drv<CM> v(drv, w.seg);
  double acc[L];
#pragma unroll
  for (int q = 0; q < L; ++q) acc[q] = 0.0;
  for (int ch = blockIdx.x; ch < w.nch; ch += gridDim.x) {
    const auto r = w.chunk(ch);
    float Areg[CM];
    load_row<CM>(A + static_cast<size_t>(r.grow) * CM, Areg);
    for (int it = 0; it < w.niter; ++it) {
      const auto s = w.step(r, it);
      const float h = hbuf[r.g * Q + s.jc];
      float z2[K2];
#pragma unroll
      for (int k = 0; k < K2; ++k) z2[k] = b2[k];
#pragma unroll
      for (int c4 = 0; c4 < CM / 4; ++c4) {
        float a4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a4[e] = Areg[4 * c4 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a1 = act1<CM>(h, a4[e], 4 * c4 + e, wh, v);
#pragma unroll
          for (int k = 0; k < K2; ++k) z2[k] = __builtin_fmaf(W2[k * CM + 4 * c4 + e], a1, z2[k]);
        }
      }
      const float duv = s.act ? du[s.pair] : 0.f;
#pragma unroll
      for (int k = 0; k < K2; ++k) {
        const Back2 b = back2<CM>(z2[k], duv, s.act, k, w3, v);
        acc[k] += b.dy2;
        acc[K2 + k] += static_cast<double>(b.dy2) * b.xh2;
        acc[2 * K2 + k] += static_cast<double>(duv) * leaky(b.y2);
      }
      acc[3 * K2] += duv;
    }
  }
  block_reduce_store<L>(acc, part + w.partial() * L);
}

// d W2, sum dy1 and sum dy1 xhat1 are sums over pairs of products of two per-pair vectors.  A wave
// lays 16 channels of its 64 pairs' xhat1 and dy1, and their dz2, out in LDS; lane (channel cl, k
// quarter kq) then sums over the 64 pairs, and keeps its sums across the block's chunks and steps.
template <int CM>
__global__ __launch_bounds__(pair_threads<CM>()) void k_b2(
    const float* __restrict__ A, const float* __restrict__ hbuf, const float* __restrict__ wh,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ g1, const float* __restrict__ be1, const float* __restrict__ drv,
    const float* __restrict__ du, double* __restrict__ part, double* __restrict__ wpart, int N, int Q,
    int want_params) {
  constexpr int K2 = CM / 4, NW = Walk<CM>::NW, L = part_len(CM).b2, WL = part_len(CM).b2w;
  constexpr int CG = 16, NGRP = CM / CG, KQ = K2 / 4;
  __shared__ float XH[NW][64][CG + 1], DY[NW][64][CG + 1], DZ[NW][64][K2 + 1];
  const Walk<CM> w(N, Q);
  const Drv<CM> v(drv, w.seg);
  const int lane = w.lane, wave = w.wave, cl = lane & (CG - 1), kq = lane >> 4;
  const size_t P = w.partial();
  double acc[L], pW[NGRP * KQ], pS[NGRP * 2];
#pragma unroll
  for (int q = 0; q < L; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < NGRP * KQ; ++q) pW[q] = 0.0;
#pragma unroll
  for (int q = 0; q < NGRP * 2; ++q) pS[q] = 0.0;
  for (int ch = blockIdx.x; ch < w.nch; ch += gridDim.x) {
    const auto r = w.chunk(ch);
    float Areg[CM];
    load_row<CM>(A + static_cast<size_t>(r.grow) * CM, Areg);
    for (int it = 0; it < w.niter; ++it) {
      const auto s = w.step(r, it);
      const float h = hbuf[r.g * Q + s.jc];
      float z2[K2], dz2[K2];
#pragma unroll
      for (int k = 0; k < K2; ++k) z2[k] = b2[k];
#pragma unroll
      for (int c4 = 0; c4 < CM / 4; ++c4) {
        float a4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a4[e] = Areg[4 * c4 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a1 = act1<CM>(h, a4[e], 4 * c4 + e, wh, v);
#pragma unroll
          for (int k = 0; k < K2; ++k) z2[k] = __builtin_fmaf(W2[k * CM + 4 * c4 + e], a1, z2[k]);
        }
      }
      const float duv = s.act ? du[s.pair] : 0.f;
#pragma unroll
      for (int k = 0; k < K2; ++k) {
        dz2[k] = back2<CM>(z2[k], duv, s.act, k, w3, v).dz2;
        acc[k] += dz2[k];
        DZ[wave][lane][k] = dz2[k];
      }
#pragma unroll
      for (int grp = 0; grp < NGRP; ++grp) {
#pragma unroll
        for (int e = 0; e < CG; ++e) {
          const int c = grp * CG + e;
          const Fwd1 f = fwd1<CM>(h, Areg[c], c, wh, v);
          float da1 = 0.f;
#pragma unroll
          for (int k = 0; k < K2; ++k) da1 = __builtin_fmaf(W2[k * CM + c], dz2[k], da1);
          XH[wave][lane][e] = (f.z1 - v.mean1[c]) * v.rstd1[c];
          DY[wave][lane][e] = da1 * leaky_slope(f.y1);
        }
        __syncthreads();
        {  // channel c = grp CG + cl, outputs k = kq KQ .. + KQ - 1 over the wave's 64 pairs
          const int c = grp * CG + cl;
          const float gam = g1[c], bet = be1[c];
          float tw[KQ], sdy = 0.f, sdyx = 0.f;
#pragma unroll
          for (int kk = 0; kk < KQ; ++kk) tw[kk] = 0.f;
          for (int p = 0; p < 64; ++p) {
            const float xh = XH[wave][p][cl], dy = DY[wave][p][cl];
            sdy += dy;
            sdyx = __builtin_fmaf(dy, xh, sdyx);
            if (want_params) {
              const float a1 = leaky(__builtin_fmaf(xh, gam, bet));
#pragma unroll
              for (int kk = 0; kk < KQ; ++kk) tw[kk] = __builtin_fmaf(DZ[wave][p][kq * KQ + kk], a1, tw[kk]);
            }
          }
#pragma unroll
          for (int kk = 0; kk < KQ; ++kk) pW[grp * KQ + kk] += tw[kk];
          pS[grp * 2] += sdy;
          pS[grp * 2 + 1] += sdyx;
        }
        __syncthreads();
      }
    }
  }
  block_reduce_store<L>(acc, part + P * L);
  double* wp = wpart + (P * NW + wave) * WL;
#pragma unroll
  for (int grp = 0; grp < NGRP; ++grp) {
    const int c = grp * CG + cl;
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) wp[(kq * KQ + kk) * CM + c] = pW[grp * KQ + kk];
    if (kq == 0) {
      wp[K2 * CM + c] = pS[grp * 2];
      wp[K2 * CM + CM + c] = pS[grp * 2 + 1];
    }
  }
}

// Keeps the lane's dA row (f64) and d w_h terms across its j, so the A row is read from memory, and
// the j slabs (grid.z) each write a dA buffer of their own (k_sum_slabs adds them in order); with one
// slab dA goes over A.
template <int CM>
__global__ __launch_bounds__(pair_threads<CM>()) void k_b3(
    float* Arw, const float* __restrict__ hbuf, const float* __restrict__ wh, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ drv,
    const float* __restrict__ du, float* __restrict__ tbuf, double* __restrict__ part, float* dAbuf, int N, int Q) {
  constexpr int K2 = CM / 4, NT = Walk<CM>::NT, NW = Walk<CM>::NW, L = part_len(CM).b3;
  __shared__ double comb[NW][64][9];  // the cross-wave sums of a chunk, eight channels at a time
  __shared__ double dwh_blk[L];       // the block's d w_h
  const Walk<CM> w(N, Q);
  const Drv<CM> v(drv, w.seg);
  const int tid = w.tid, lane = w.lane, wave = w.wave, NQ = w.NQ;
  for (int c = tid; c < CM; c += NT) dwh_blk[c] = 0.0;
  __syncthreads();
  for (int ch = blockIdx.x; ch < w.nch; ch += gridDim.x) {
    const auto r = w.chunk(ch);
    const float* Arow = Arw + static_cast<size_t>(r.grow) * CM;
    double dA[CM];
    float dwh[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      dA[c] = 0.0;
      dwh[c] = 0.f;
    }
    for (int it = 0; it < w.niter; ++it) {
      const auto s = w.step(r, it);
      const float h = hbuf[r.g * Q + s.jc];
      float z2[K2], dz2[K2];
#pragma unroll
      for (int k = 0; k < K2; ++k) z2[k] = b2[k];
#pragma unroll
      for (int c4 = 0; c4 < CM / 4; ++c4) {
        float a4[4];
        load_row<4>(Arow + 4 * c4, a4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a1 = act1<CM>(h, a4[e], 4 * c4 + e, wh, v);
#pragma unroll
          for (int k = 0; k < K2; ++k) z2[k] = __builtin_fmaf(W2[k * CM + 4 * c4 + e], a1, z2[k]);
        }
      }
      const float duv = s.act ? du[s.pair] : 0.f;
#pragma unroll
      for (int k = 0; k < K2; ++k) dz2[k] = back2<CM>(z2[k], duv, s.act, k, w3, v).dz2;
      float ts = 0.f;
#pragma unroll
      for (int c4 = 0; c4 < CM / 4; ++c4) {
        float a4[4];
        load_row<4>(Arow + 4 * c4, a4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * c4 + e;
          const Fwd1 f = fwd1<CM>(h, a4[e], c, wh, v);
          float da1 = 0.f;
#pragma unroll
          for (int k = 0; k < K2; ++k) da1 = __builtin_fmaf(W2[k * CM + c], dz2[k], da1);
          const float dy1 = da1 * leaky_slope(f.y1);
          const float xh1 = (f.z1 - v.mean1[c]) * v.rstd1[c];
          const float dz1 = s.act ? v.sc1[c] * (dy1 - v.m1a[c] - xh1 * v.m1b[c]) : 0.f;
          dA[c] += dz1;
          dwh[c] = __builtin_fmaf(dz1, h, dwh[c]);
          ts = __builtin_fmaf(dz1, wh[c], ts);
        }
      }
      if (s.act) tbuf[s.pair] = ts;
    }
    // the chunk's dA rows: the waves' sums over their j added in wave order (one slab: every wave is
    // past its last read of these rows at the first barrier); d w_h: lanes, then waves
    float* Ao = dAbuf ? dAbuf + static_cast<size_t>(blockIdx.z) * gridDim.y * NQ * CM : Arw;
#pragma unroll
    for (int g8 = 0; g8 < CM / 8; ++g8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) comb[wave][lane][e] = dA[g8 * 8 + e];
      __syncthreads();
      for (int o = tid; o < 512; o += NT) {
        const int l = o >> 3, e = o & 7, row = ch * 64 + l;
        double sum = 0.0;
        for (int ww = 0; ww < NW; ++ww) sum += comb[ww][l][e];
        if (row < NQ) Ao[(static_cast<size_t>(w.seg) * NQ + row) * CM + g8 * 8 + e] = static_cast<float>(sum);
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 8; ++e) comb[wave][lane][e] = dwh[g8 * 8 + e];
      __syncthreads();
      if (tid < 8) {
        double sum = 0.0;
        for (int ww = 0; ww < NW; ++ww)
          for (int l = 0; l < 64; ++l) sum += comb[ww][l][tid];
        dwh_blk[g8 * 8 + tid] += sum;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int c = tid; c < CM; c += NT) part[w.partial() * L + c] = dwh_blk[c];
}

// ------------------------------------------------------------------ finalisers
// BN2: from k_stats' partials (training) or the running statistics.  One block per segment.
template <int CM>
__global__ void k_fin_bn2(const double* __restrict__ part, int nparts, int N, int Q, const float* __restrict__ g2,
                          const float* __restrict__ be2, const float* __restrict__ rm2,
                          const float* __restrict__ rv2, int training, float eps, float* __restrict__ drv,
                          float* __restrict__ stats) {
  constexpr int K2 = CM / 4, L = part_len(CM).stats;
  const int seg = blockIdx.x, k = threadIdx.x;
  if (k >= K2) return;
  double a1 = 0.0, a2 = 0.0;
  if (training) {
    for (int p = 0; p < nparts; ++p) {
      const double* pp = part + (static_cast<size_t>(seg) * nparts + p) * L;
      a1 += pp[k];
      a2 += pp[K2 + k];
    }
  }
  bn_finish<CM>(training, a1, a2, static_cast<double>(N) * Q * Q, rm2, rv2, g2, be2, k, eps, stats, seg, CM + k,
                Drv<CM>::bn2(drv, seg, D_SC) + k, K2);
}

// dparams layout (floats): W1 [cm (C + 1)] | gamma1 | beta1 [cm] | W2 [K2 cm] | b2 | gamma2 | beta2 | w3 [K2] | b3 [1]
struct DpOff {
  long long w1, g1, be1, w2, b2, g2, be2, w3, b3, total;
};
inline DpOff dp_off(int C, int cm) {
  DpOff o;
  const int k2 = cm / 4;
  o.w1 = 0;
  o.g1 = static_cast<long long>(cm) * (C + 1);
  o.be1 = o.g1 + cm;
  o.w2 = o.be1 + cm;
  o.b2 = o.w2 + static_cast<long long>(k2) * cm;
  o.g2 = o.b2 + k2;
  o.be2 = o.g2 + k2;
  o.w3 = o.be2 + k2;
  o.b3 = o.w3 + k2;
  o.total = o.b3 + 1;
  return o;
}

// k_b1: the per-segment means BN2's backward needs (training) and d gamma2, d beta2, d w3, d b3 summed
// over the segments in order.  One block, thread k (thread K2: d b3).
template <int CM>
__global__ void k_fin_b1(const double* __restrict__ part, int S, int nparts, int N, int Q, int training,
                         float* __restrict__ drv, float* __restrict__ dp, DpOff o) {
  constexpr int K2 = CM / 4, L = part_len(CM).b1;
  const int k = threadIdx.x;
  if (k > K2) return;
  const double M = static_cast<double>(N) * Q * Q;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  for (int seg = 0; seg < S; ++seg) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int p = 0; p < nparts; ++p) {
      const double* pp = part + (static_cast<size_t>(seg) * nparts + p) * L;
      if (k == K2) {
        a0 += pp[3 * K2];
      } else {
        a0 += pp[k];
        a1 += pp[K2 + k];
        a2 += pp[2 * K2 + k];
      }
    }
    if (k < K2 && training) {
      Drv<CM>::bn2(drv, seg, D_MA)[k] = static_cast<float>(a0 / M);
      Drv<CM>::bn2(drv, seg, D_MB)[k] = static_cast<float>(a1 / M);
    }
    t0 += a0;
    t1 += a1;
    t2 += a2;
  }
  if (!dp) return;
  if (k == K2) {
    dp[o.b3] = static_cast<float>(t0);
  } else {
    dp[o.be2 + k] = static_cast<float>(t0);
    dp[o.g2 + k] = static_cast<float>(t1);
    dp[o.w3 + k] = static_cast<float>(t2);
  }
}

// k_b2: output q of [d W2 (K2 cm) | sum dy1 (cm) | sum dy1 xhat1 (cm) | d b2 (K2)].  A block = 64 outputs x 4
// groups; group r adds the partials p = r mod 4 in order, then the four groups are added in order.
template <int CM>
__global__ __launch_bounds__(256) void k_fin_b2(const double* __restrict__ part, const double* __restrict__ wpart,
                                                int S, int nparts, int nwparts, int N, int Q, int training,
                                                float* __restrict__ drv, float* __restrict__ dp, DpOff o) {
  constexpr int K2 = CM / 4, L = part_len(CM).b2, WL = part_len(CM).b2w;
  __shared__ double sm[4][64];
  const int ql = threadIdx.x & 63, grp = threadIdx.x >> 6, q = blockIdx.x * 64 + ql;
  const bool ok = q < WL + L;
  const double M = static_cast<double>(N) * Q * Q;
  double tot = 0.0;
  for (int seg = 0; seg < S; ++seg) {
    double a = 0.0;
    if (ok) {
      if (q < WL) {
        for (int p = grp; p < nwparts; p += 4) a += wpart[(static_cast<size_t>(seg) * nwparts + p) * WL + q];
      } else {
        for (int p = grp; p < nparts; p += 4) a += part[(static_cast<size_t>(seg) * nparts + p) * L + (q - WL)];
      }
    }
    sm[grp][ql] = a;
    __syncthreads();
    if (grp == 0 && ok) {
      a = ((sm[0][ql] + sm[1][ql]) + sm[2][ql]) + sm[3][ql];
      if (training && q >= K2 * CM && q < WL) {
        const int c = (q - K2 * CM) % CM;  // sum dy1 [cm] | sum dy1 xhat1 [cm]
        Drv<CM>::bn1(drv, seg, q < K2 * CM + CM ? D_MA : D_MB)[c] = static_cast<float>(a / M);
      }
      tot += a;
    }
    __syncthreads();
  }
  if (!dp || grp != 0 || !ok) return;
  if (q < K2 * CM) dp[o.w2 + q] = static_cast<float>(tot);
  else if (q < K2 * CM + CM) dp[o.be1 + (q - K2 * CM)] = static_cast<float>(tot);
  else if (q < WL) dp[o.g1 + (q - K2 * CM - CM)] = static_cast<float>(tot);
  else dp[o.b2 + (q - WL)] = static_cast<float>(tot);
}

// k_b3: d w_h = column 0 of d W1
__global__ void k_fin_b3(const double* __restrict__ part, int nparts_all, int cm, int ldw, float* __restrict__ dp) {
  const int c = threadIdx.x;
  if (c >= cm) return;
  double a = 0.0;
  for (int p = 0; p < nparts_all; ++p) a += part[static_cast<size_t>(p) * cm + c];
  dp[static_cast<size_t>(c) * ldw] = static_cast<float>(a);
}

// d W_f[c][ch] = sum over all rows of dA[row][c] F_s[row][ch]: block (8 channels, row slab), thread
// (c, channel group) sums its slab's rows in order in f64 into pd[slab][ch][c]; k_fin_dw1 adds the slabs.
constexpr int kDw1Slabs = 8;
template <typename T, int CM>
__global__ __launch_bounds__(256) void k_dw1(const float* __restrict__ dA, const T* __restrict__ feat,
                                             const int* __restrict__ idx, int rows, int Q, int HW, int C,
                                             double* __restrict__ pd) {
  constexpr int NG = 256 / CM, EPT = 8 / NG;  // channel groups per block, channels per thread
  const int tid = threadIdx.x, c = tid % CM, eg = tid / CM, ch0 = blockIdx.x * 8 + eg * EPT;
  const int per = (rows + gridDim.y - 1) / gridDim.y, r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
  double acc[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) acc[e] = 0.0;
#pragma unroll 4
  for (int row = r0; row < r1; ++row) {
    const int g = row / Q, pos = sample_pos(idx, row, HW);
    const double a = dA[static_cast<size_t>(row) * CM + c];
    const size_t fo = (static_cast<size_t>(g) * HW + pos) * C + ch0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] += a * static_cast<double>(ldf<T>(feat, fo + e));
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) pd[(static_cast<size_t>(blockIdx.y) * C + ch0 + e) * CM + c] = acc[e];
}
__global__ void k_fin_dw1(const double* __restrict__ pd, int slabs, int C, int cm, float* __restrict__ dp) {
  const int o = blockIdx.x * 256 + threadIdx.x;  // o = ch * cm + c
  if (o >= C * cm) return;
  double a = 0.0;
  for (int s = 0; s < slabs; ++s) a += pd[static_cast<size_t>(s) * C * cm + o];
  const int ch = o / cm, c = o - ch * cm;
  dp[static_cast<size_t>(c) * (C + 1) + 1 + ch] = static_cast<float>(a);
}

// A[i] = the j slabs' dA buffers added in slab order
__global__ void k_sum_slabs(const float* __restrict__ buf, int slabs, long long n, float* __restrict__ A) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  float s = buf[i];
  for (int z = 1; z < slabs; ++z) s += buf[z * n + i];
  A[i] = s;
}

// dh[g, j] = sum_i t[g, i, j]
__global__ void k_dh(const float* __restrict__ t, int rows, int Q, float* __restrict__ dh) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int g = r / Q, j = r - g * Q;
  double s = 0.0;
  for (int i = 0; i < Q; ++i) s += t[(static_cast<size_t>(g) * Q + i) * Q + j];
  dh[r] = static_cast<float>(s);
}

// Feature gradient rows: block = row (g, i).  Only the first occurrence of a position writes, with
// the sum of dA over every occurrence (in index order) times W_f.  dfeat was zeroed before.
template <typename T, int CM>
__global__ __launch_bounds__(128) void k_scatter_feat(const float* __restrict__ dA, const int* __restrict__ idx,
                                                      const float* __restrict__ W1, int Q, int HW, int C,
                                                      T* __restrict__ dfeat) {
  __shared__ float ds[CM];
  __shared__ int dup;
  const int row = blockIdx.x, g = row / Q, i = row - g * Q, tid = threadIdx.x;
  const int pos = sample_pos(idx, row, HW);
  if (tid == 0) dup = 0;
  __syncthreads();
  for (int k = tid; k < i; k += 128)
    if (sample_pos(idx, g * Q + k, HW) == pos) dup = 1;
  __syncthreads();
  if (dup) return;
  if (tid < CM) {
    float s = dA[static_cast<size_t>(row) * CM + tid];
    for (int k = i + 1; k < Q; ++k)
      if (sample_pos(idx, g * Q + k, HW) == pos) s += dA[(static_cast<size_t>(g) * Q + k) * CM + tid];
    ds[tid] = s;
  }
  __syncthreads();
  for (int ch = tid; ch < C; ch += 128) {
    float s = 0.f;
#pragma unroll 8
    for (int c = 0; c < CM; ++c) s = __builtin_fmaf(ds[c], W1[static_cast<size_t>(c) * (C + 1) + 1 + ch], s);
    stf(dfeat, (static_cast<size_t>(g) * HW + pos) * C + ch, s);
  }
}

__global__ void k_scatter_hm(const float* __restrict__ dh, const int* __restrict__ idx, int rows, int Q, int HW,
                             int J, int joint, float* __restrict__ dhm) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int g = r / Q, j = r - g * Q, pos = sample_pos(idx, r, HW);
  for (int k = 0; k < j; ++k)
    if (sample_pos(idx, g * Q + k, HW) == pos) return;
  float s = dh[r];
  for (int k = j + 1; k < Q; ++k)
    if (sample_pos(idx, g * Q + k, HW) == pos) s += dh[g * Q + k];
  dhm[(static_cast<size_t>(g) * J + joint) * HW + pos] = s;
}

// ------------------------------------------------------------------ the measures on u
__device__ __forceinline__ float softplus_neg(float x) {  // softplus(-x), stable for |x| large
  return fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoidf(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
constexpr float kLog2 = 0.69314718055994530942f;
constexpr float kNceMask = -10.f;

// NCE over row i's [u_ii, u_i0 .. u_i,Q-1 with -10 at j = i]: the maximum m and the sum s of exp(. - m)
struct NceRow {
  float m, s;
};
__device__ __forceinline__ NceRow nce_row(const float* __restrict__ ur, int i, int Q) {
  const float up = ur[i];
  float m = up;
  for (int j = 0; j < Q; ++j) m = fmaxf(m, j == i ? kNceMask : ur[j]);
  float s = expf(up - m);
  for (int j = 0; j < Q; ++j) s += expf((j == i ? kNceMask : ur[j]) - m);
  return {m, s};
}

// thread = row (n, i) of the segment.  JSD: acc0 = sum over the diagonal of log 2 - softplus(-u),
// acc1 = sum off the diagonal of softplus(-u) + u - log 2.  NCE: acc0 = sum of lse - u_ii.
__global__ __launch_bounds__(256) void k_mi_fwd(const float* __restrict__ u, int N, int Q, int measure,
                                                double* __restrict__ part) {
  const int seg = blockIdx.y, NQ = N * Q;
  double acc[2] = {0.0, 0.0};
  for (int r = blockIdx.x * 256 + threadIdx.x; r < NQ; r += gridDim.x * 256) {
    const int i = r % Q;
    const float* ur = u + (static_cast<size_t>(seg) * NQ + r) * Q;
    if (measure == 0) {
      double neg = 0.0;
      for (int j = 0; j < Q; ++j) {
        const float v = ur[j], sp = softplus_neg(v);
        if (j == i) acc[0] += kLog2 - sp;
        else neg += (sp + v) - kLog2;
      }
      acc[1] += neg;
    } else {
      const NceRow n = nce_row(ur, i, Q);
      acc[0] += static_cast<double>(n.m + logf(n.s)) - ur[i];
    }
  }
  block_reduce_store<2>(acc, part + (static_cast<size_t>(seg) * gridDim.x + blockIdx.x) * 2);
}

__global__ void k_mi_fin(const double* __restrict__ part, int S, int nparts, int N, int Q, int measure,
                         float* __restrict__ loss) {
  for (int seg = threadIdx.x; seg < S; seg += blockDim.x) {
    double a0 = 0.0, a1 = 0.0;
    for (int p = 0; p < nparts; ++p) {
      a0 += part[(static_cast<size_t>(seg) * nparts + p) * 2];
      a1 += part[(static_cast<size_t>(seg) * nparts + p) * 2 + 1];
    }
    const double NQ = static_cast<double>(N) * Q;
    loss[seg] = static_cast<float>(measure == 0 ? a1 / (NQ * (Q - 1)) - a0 / NQ : a0 / NQ);
  }
}

__global__ __launch_bounds__(256) void k_mi_bwd(const float* __restrict__ u, int S, int N, int Q, int measure,
                                                const float* __restrict__ gloss, float* __restrict__ du) {
  const int NQ = N * Q, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= S * NQ) return;
  const int seg = r / NQ, i = r % Q;
  const float gl = gloss[seg];
  const float* ur = u + static_cast<size_t>(r) * Q;
  float* dr = du + static_cast<size_t>(r) * Q;
  if (measure == 0) {
    const float wp = -gl / static_cast<float>(NQ);
    const float wn = gl / (static_cast<float>(NQ) * static_cast<float>(Q - 1));
    for (int j = 0; j < Q; ++j) dr[j] = j == i ? wp * sigmoidf(-ur[j]) : wn * sigmoidf(ur[j]);
  } else {
    const float up = ur[i], w = gl / static_cast<float>(NQ);
    const NceRow n = nce_row(ur, i, Q);
    const float inv = 1.f / n.s;
    for (int j = 0; j < Q; ++j) dr[j] = j == i ? w * (expf(up - n.m) * inv - 1.f) : w * expf(ur[j] - n.m) * inv;
  }
}

// ------------------------------------------------------------------ host side
// Launch geometry of a shape
struct Shape {
  int S, N, Q, cm, rows, nch, NW, NB, JS, JS3;
  int np, np3, nwp;  // partial blocks per segment (k_stats / k_b1 / k_b2), of k_b3, per-wave of k_b2
};

bool make_shape(int S, int N, int Q, int cm, Shape* sh) {
  if (S < 1 || N < 1 || Q < 1 || Q > 256) return false;
  if (cm != 32 && cm != 64 && cm != 128) return false;
  if (static_cast<long long>(S) * N * Q * Q * cm >= (1ll << 31)) return false;
  Shape& s = *sh;
  s.S = S, s.N = N, s.Q = Q, s.cm = cm;
  s.rows = S * N * Q;
  s.nch = (N * Q + 63) / 64;
  s.NW = cm == 128 ? 2 : 4;
  s.NB = std::min(s.nch, kMaxNB);
  s.JS = std::max(1, std::min(kMaxJS, Q / 8));
  // k_b3's slabs each own a dA buffer: as many as fit in two floats per pair
  s.JS3 = s.JS;
  while (s.JS3 > 1 && static_cast<long long>(s.JS3) * cm > 2ll * Q) --s.JS3;
  s.np = s.NB * s.JS;
  s.np3 = s.NB * s.JS3;
  s.nwp = s.np * s.NW;
  return true;
}

// The workspace: its regions in order, each 16-byte aligned where its element type changes.  With
// ws = nullptr only the sizes are meaningful.
struct Ws {
  float *A, *h, *dh, *t, *dAbuf, *wh, *drv;
  double *p_stats, *p_b1, *p_b2, *p_b2w, *p_b3, *p_dw1;
  long long bytes, red_bytes;  // in all; of it what does not grow with the pairs
};
Ws carve(void* ws, const Shape& s) {
  Ws w;
  long long off = 0;
  auto take = [&](auto*& p, long long count) {
    using T = std::remove_reference_t<decltype(*p)>;
    p = count ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(ws) + off) : nullptr;
    off += count * static_cast<long long>(sizeof(T));
  };
  auto align16 = [&] { off = (off + 15) / 16 * 16; };
  const long long rows = s.rows, M = rows * s.Q, S = s.S, cm = s.cm;
  const PartLen len = part_len(s.cm);
  // A | h | dh | t | k_b3's slab buffers: S N Q (cm + 2) + S N Q^2 (+ JS3 S N Q cm <= 2 S N Q^2) floats
  take(w.A, rows * cm);
  take(w.h, rows);
  take(w.dh, rows);
  take(w.t, M);
  take(w.dAbuf, s.JS3 > 1 ? s.JS3 * rows * cm : 0);
  align16();
  // what does not grow with the pairs: w_h, the derived per-segment values, the f64 partials
  const long long fixed = off;
  take(w.wh, cm);
  take(w.drv, S * drv_stride(s.cm));
  const long long drv_bytes = off - fixed;
  align16();
  const long long base = off;
  take(w.p_stats, S * s.np * len.stats);
  take(w.p_b1, S * s.np * len.b1);
  take(w.p_b2, S * s.np * len.b2);
  take(w.p_b2w, S * s.nwp * len.b2w);
  take(w.p_b3, S * s.np3 * len.b3);
  take(w.p_dw1, static_cast<long long>(kDw1Slabs) * 512 * cm);  // C <= 512
  w.bytes = off;
  w.red_bytes = off - base + drv_bytes + 32;
  return w;
}

struct Args {
  int dtype;
  const void* feat;
  const float* hm;
  int S, N, H, W, C, J, joint;
  const int* idx;
  const int* idx_host;
  int Q, cm;
  const float* const* params;
  int training;
};

int validate(const char* fn, const Args& a, const void* ws, long long ws_bytes, Shape* sh) {
  const std::string f(fn);
  POSU_REQUIRE(a.dtype == POSU_F32 || a.dtype == POSU_BF16 || a.dtype == POSU_F16,
               f + ": features must be POSU_F32, POSU_BF16 or POSU_F16");
  POSU_REQUIRE(a.cm == 32 || a.cm == 64 || a.cm == 128, f + ": c_m must be 32, 64 or 128");
  POSU_REQUIRE(a.C >= 8 && a.C % 8 == 0 && a.C <= 512, f + ": C must be a multiple of 8, at most 512");
  POSU_REQUIRE(a.Q >= 1 && a.Q <= 256, f + ": Q must be in 1..256");
  POSU_REQUIRE(a.S >= 1 && a.N >= 1 && a.H >= 1 && a.W >= 1 && a.J >= 1, f + ": non-positive size");
  POSU_REQUIRE(a.joint >= 0 && a.joint < a.J, f + ": joint_idx out of range");
  const long long HW = static_cast<long long>(a.H) * a.W;
  POSU_REQUIRE(static_cast<long long>(a.S) * a.N * HW * std::max(a.C, a.J) < (1ll << 31), f + ": shape too large");
  POSU_REQUIRE(static_cast<long long>(a.S) * a.N * a.Q * a.Q * a.cm < (1ll << 31),
               f + ": shape too large (M * c_m must stay below 2^31)");
  POSU_REQUIRE(a.feat && a.hm && a.idx && a.params && ws, f + ": null pointer");
  for (int p = 0; p < P_COUNT; ++p) {
    const bool running = p == P_RM1 || p == P_RV1 || p == P_RM2 || p == P_RV2;
    POSU_REQUIRE(a.params[p] || (running && a.training), f + ": null pointer (parameter table)");
  }
  if (a.idx_host) {
    const long long n = static_cast<long long>(a.S) * a.N * a.Q;
    for (long long k = 0; k < n; ++k)
      POSU_REQUIRE(a.idx_host[k] >= 0 && a.idx_host[k] < HW, f + ": index outside [0, H*W)");
  }
  POSU_REQUIRE(make_shape(a.S, a.N, a.Q, a.cm, sh), f + ": shape too large");
  POSU_REQUIRE(ws_bytes >= carve(nullptr, *sh).bytes, f + ": workspace too small");
  POSU_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, f + ": workspace must be 16-byte aligned");
  return POSU_OK;
}

dim3 pair_grid(const Shape& s, int js) { return dim3(s.NB, s.S, js); }

// gather + BN1 + (training) the BN2 statistics pass: everything k_score and the backward passes need
template <typename T, int CM>
int prepare(const char* fn, const Args& a, const Shape& s, const Ws& w, float eps, float* stats, hipStream_t st) {
  const float* const* p = a.params;
  k_gather<T, CM><<<(s.rows + kGatherRows - 1) / kGatherRows, 256, 0, st>>>(
      static_cast<const T*>(a.feat), a.hm, a.idx, p[P_W1], s.rows, s.Q, a.H * a.W, a.C, a.J, a.joint, w.A, w.h, w.wh);
  if (int e = check_launch(fn)) return e;
  k_bn1<CM><<<s.S, 256, 0, st>>>(w.A, w.h, w.wh, p[P_G1], p[P_BE1], p[P_RM1], p[P_RV1], s.N, s.Q, a.training, eps,
                                 w.drv, stats);
  if (int e = check_launch(fn)) return e;
  if (a.training) {
    k_stats<CM><<<pair_grid(s, s.JS), pair_threads<CM>(), 0, st>>>(w.A, w.h, w.wh, p[P_W2], p[P_B2], w.drv,
                                                                      w.p_stats, s.N, s.Q);
    if (int e = check_launch(fn)) return e;
  }
  k_fin_bn2<CM><<<s.S, 64, 0, st>>>(w.p_stats, s.np, s.N, s.Q, p[P_G2], p[P_BE2], p[P_RM2], p[P_RV2], a.training, eps,
                                    w.drv, stats);
  return check_launch(fn);
}

template <typename T, int CM>
int run_fwd(const char* fn, const Args& a, const Shape& s, void* ws, float eps, float* stats, float* u,
            hipStream_t st) {
  const Ws w = carve(ws, s);
  const float* const* p = a.params;
  if (int e = prepare<T, CM>(fn, a, s, w, eps, stats, st)) return e;
  k_score<CM><<<pair_grid(s, s.JS), pair_threads<CM>(), 0, st>>>(w.A, w.h, w.wh, p[P_W2], p[P_B2], p[P_W3], p[P_B3],
                                                                    w.drv, u, s.N, s.Q);
  return check_launch(fn);
}

template <typename T, int CM>
int run_bwd(const char* fn, const Args& a, const Shape& s, void* ws, float eps, float* stats, const float* du,
            float* dp, void* dfeat, float* dhm, hipStream_t st) {
  const Ws w = carve(ws, s);
  const float* const* p = a.params;
  const DpOff o = dp_off(a.C, a.cm);
  const int HW = a.H * a.W;
  constexpr int NT = pair_threads<CM>();
  if (int e = prepare<T, CM>(fn, a, s, w, eps, stats, st)) return e;
  k_b1<CM><<<pair_grid(s, s.JS), NT, 0, st>>>(w.A, w.h, w.wh, p[P_W2], p[P_B2], p[P_W3], w.drv, du, w.p_b1, s.N,
                                                 s.Q);
  if (int e = check_launch(fn)) return e;
  k_fin_b1<CM><<<1, 64, 0, st>>>(w.p_b1, s.S, s.np, s.N, s.Q, a.training, w.drv, dp, o);
  if (int e = check_launch(fn)) return e;
  k_b2<CM><<<pair_grid(s, s.JS), NT, 0, st>>>(w.A, w.h, w.wh, p[P_W2], p[P_B2], p[P_W3], p[P_G1], p[P_BE1], w.drv,
                                                 du, w.p_b2, w.p_b2w, s.N, s.Q, dp != nullptr);
  if (int e = check_launch(fn)) return e;
  constexpr int nq = part_len(CM).b2w + part_len(CM).b2;
  k_fin_b2<CM><<<(nq + 63) / 64, 256, 0, st>>>(w.p_b2, w.p_b2w, s.S, s.np, s.nwp, s.N, s.Q, a.training, w.drv, dp, o);
  if (int e = check_launch(fn)) return e;
  k_b3<CM><<<pair_grid(s, s.JS3), NT, 0, st>>>(w.A, w.h, w.wh, p[P_W2], p[P_B2], p[P_W3], w.drv, du, w.t, w.p_b3,
                                                  w.dAbuf, s.N, s.Q);  // A becomes dA
  if (int e = check_launch(fn)) return e;
  if (w.dAbuf) {
    const long long n = static_cast<long long>(s.rows) * a.cm;
    k_sum_slabs<<<static_cast<unsigned>((n + 255) / 256), 256, 0, st>>>(w.dAbuf, s.JS3, n, w.A);
    if (int e = check_launch(fn)) return e;
  }
  if (dp) {
    k_fin_b3<<<1, 128, 0, st>>>(w.p_b3, s.S * s.np3, a.cm, a.C + 1, dp + o.w1);
    if (int e = check_launch(fn)) return e;
    const int slabs = std::min(kDw1Slabs, (s.rows + 255) / 256);
    k_dw1<T, CM><<<dim3(a.C / 8, slabs), 256, 0, st>>>(w.A, static_cast<const T*>(a.feat), a.idx, s.rows, s.Q, HW, a.C,
                                                      w.p_dw1);
    if (int e = check_launch(fn)) return e;
    k_fin_dw1<<<(a.C * a.cm + 255) / 256, 256, 0, st>>>(w.p_dw1, slabs, a.C, a.cm, dp + o.w1);
    if (int e = check_launch(fn)) return e;
  }
  if (dfeat) {
    const size_t bytes = static_cast<size_t>(a.S) * a.N * HW * a.C * sizeof(T);
    if (hipMemsetAsync(dfeat, 0, bytes, st) != hipSuccess) return check_launch(fn);
    k_scatter_feat<T, CM><<<s.rows, 128, 0, st>>>(w.A, a.idx, p[P_W1], s.Q, HW, a.C, static_cast<T*>(dfeat));
    if (int e = check_launch(fn)) return e;
  }
  if (dhm) {
    const size_t bytes = static_cast<size_t>(a.S) * a.N * a.J * HW * sizeof(float);
    if (hipMemsetAsync(dhm, 0, bytes, st) != hipSuccess) return check_launch(fn);
    k_dh<<<(s.rows + 255) / 256, 256, 0, st>>>(w.t, s.rows, s.Q, w.dh);
    if (int e = check_launch(fn)) return e;
    k_scatter_hm<<<(s.rows + 255) / 256, 256, 0, st>>>(w.dh, a.idx, s.rows, s.Q, HW, a.J, a.joint, dhm);
    if (int e = check_launch(fn)) return e;
  }
  return POSU_OK;
}

// What both pair-score entry points do around their launches: the argument and shape checks, those of
// `io` (u or du), `stats` and the BatchNorm rows, then run(T{}, c_m constant, shape) under the
// feature type and c_m of the call; `nothing`: every check, no launch.
template <typename Run>
int pair_scores(const char* fn, const Args& a, const void* io, const float* stats, void* ws, long long ws_bytes,
                bool nothing, Run&& run) {
  const std::string f(fn);
  Shape s;
  if (int e = validate(fn, a, ws, ws_bytes, &s)) return e;
  POSU_REQUIRE(io && (stats || !a.training), f + ": null pointer");
  POSU_REQUIRE(!a.training || static_cast<long long>(a.N) * a.Q * a.Q > 1,
               f + ": training-mode BatchNorm needs more than one row per segment");
  if (nothing) return POSU_OK;
  int st = POSU_OK;
  with_storage(a.dtype, [&](auto tag) {
    switch (a.cm) {
      case 32: st = run(tag, std::integral_constant<int, 32>{}, s); break;
      case 64: st = run(tag, std::integral_constant<int, 64>{}, s); break;
      default: st = run(tag, std::integral_constant<int, 128>{}, s); break;
    }
  });
  return st;
}

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" long long posu_heatmap_mi_workspace(int S, int N, int Q, int cm, long long* reduction_bytes) {
  Shape s;
  if (!make_shape(S, N, Q, cm, &s)) return -1;
  const Ws w = carve(nullptr, s);
  if (reduction_bytes) *reduction_bytes = w.red_bytes;
  return w.bytes;
}

extern "C" long long posu_heatmap_dparams_floats(int C, int cm) {
  if (C < 1 || (cm != 32 && cm != 64 && cm != 128)) return -1;
  return dp_off(C, cm).total;
}

extern "C" int posu_heatmap_pair_scores_fwd(int dtype, const void* feat, const float* hm, int S, int N, int H, int W,
                                            int C, int J, int joint_idx, const int* idx, const int* idx_host, int Q,
                                            int cm, const float* const* params, int training, float eps, float* stats,
                                            float* u, void* workspace, long long workspace_bytes, void* stream) {
  const char* fn = "posu_heatmap_pair_scores_fwd";
  const Args a = {dtype, feat, hm, S, N, H, W, C, J, joint_idx, idx, idx_host, Q, cm, params, training};
  return pair_scores(fn, a, u, stats, workspace, workspace_bytes, false, [&](auto tag, auto c, const Shape& s) {
    return run_fwd<decltype(tag), decltype(c)::value>(fn, a, s, workspace, eps, stats, u, as_stream(stream));
  });
}

extern "C" int posu_heatmap_pair_scores_bwd(int dtype, const void* feat, const float* hm, int S, int N, int H, int W,
                                            int C, int J, int joint_idx, const int* idx, const int* idx_host, int Q,
                                            int cm, const float* const* params, int training, float eps,
                                            float* stats, const float* du, float* dparams, void* dfeat, float* dhm,
                                            void* workspace, long long workspace_bytes, void* stream) {
  const char* fn = "posu_heatmap_pair_scores_bwd";
  const Args a = {dtype, feat, hm, S, N, H, W, C, J, joint_idx, idx, idx_host, Q, cm, params, training};
  return pair_scores(fn, a, du, stats, workspace, workspace_bytes, !dparams && !dfeat && !dhm,
                     [&](auto tag, auto c, const Shape& s) {
                       return run_bwd<decltype(tag), decltype(c)::value>(fn, a, s, workspace, eps, stats, du, dparams,
                                                                         dfeat, dhm, as_stream(stream));
                     });
}

extern "C" long long posu_pair_mi_workspace(int S) {
  return S < 1 ? -1 : static_cast<long long>(S) * kMiNB * 2 * 8;
}

static int mi_validate(const char* fn, const void* u, int S, int N, int Q, int measure) {
  const std::string f(fn);
  POSU_REQUIRE(S >= 1 && N >= 1 && Q >= 1, f + ": non-positive size");
  POSU_REQUIRE(measure == 0 || measure == 1, f + ": measure must be 0 (JSD) or 1 (NCE)");
  POSU_REQUIRE(measure == 1 || Q >= 2, f + ": JSD needs Q >= 2 (no off-diagonal pairs otherwise)");
  POSU_REQUIRE(static_cast<long long>(S) * N * Q * Q < (1ll << 31), f + ": shape too large");
  POSU_REQUIRE(u != nullptr, f + ": null pointer");
  return POSU_OK;
}

extern "C" int posu_pair_mi_loss_fwd(const float* u, int S, int N, int Q, int measure, float* loss, void* workspace,
                                     long long workspace_bytes, void* stream) {
  if (int e = mi_validate("posu_pair_mi_loss_fwd", u, S, N, Q, measure)) return e;
  POSU_REQUIRE(loss && workspace, "posu_pair_mi_loss_fwd: null pointer");
  POSU_REQUIRE(workspace_bytes >= posu_pair_mi_workspace(S), "posu_pair_mi_loss_fwd: workspace too small");
  const int nb = std::min(kMiNB, (N * Q + 255) / 256);
  double* part = static_cast<double*>(workspace);
  k_mi_fwd<<<dim3(nb, S), 256, 0, as_stream(stream)>>>(u, N, Q, measure, part);
  if (int e = check_launch("posu_pair_mi_loss_fwd")) return e;
  k_mi_fin<<<1, 64, 0, as_stream(stream)>>>(part, S, nb, N, Q, measure, loss);
  return check_launch("posu_pair_mi_loss_fwd");
}

extern "C" int posu_pair_mi_loss_bwd(const float* u, int S, int N, int Q, int measure, const float* gloss, float* du,
                                     void* stream) {
  if (int e = mi_validate("posu_pair_mi_loss_bwd", u, S, N, Q, measure)) return e;
  POSU_REQUIRE(gloss && du, "posu_pair_mi_loss_bwd: null pointer");
  const int rows = S * N * Q;
  k_mi_bwd<<<(rows + 255) / 256, 256, 0, as_stream(stream)>>>(u, S, N, Q, measure, gloss, du);
  return check_launch("posu_pair_mi_loss_bwd");
}
