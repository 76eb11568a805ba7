// Training-mode BatchNorm2d on NHWC activations (BASELINE configs[3] training step):
// batch statistics per segment (the reference runs the backbone once per camera view,
// multiview_pose_resnet.py:74-78, so every view has its own statistics; here the views
// are stacked along the batch as `nseg` segments of `Pseg` pixels and one launch
// serves all of them), the normalise + residual + ReLU epilogue, the matching
// backward, the bias-gradient channel sum and the stem max-pool backward.
//
// Reductions are deterministic: per-block partial sums in f64 written to a workspace,
// then a data-independent order (lanes over blocks, then the lanes in order) per channel.  Running statistics
// follow torch.nn.BatchNorm2d: biased variance for normalisation, unbiased variance in
// running_var, running = (1 - momentum) * running + momentum * batch, updated once per
// segment in segment (= view) order like the reference's four backbone calls.
//
// Kernels that the tests hold bit-equal to each other (generic / segment-major apply, the
// three ReLU mask sources, the fused stem pool against apply + pool) share their arithmetic
// through the helpers of the first section: every fused multiply-add is explicit (__builtin_fmaf,
// or fma_chunk on pairs), everything else a plain operator, and an arithmetic result is an f32
// value of its own before bn_dz's products are converted (pack_results), so the equality is a property of the
// source and not of how the compiler contracts each copy.
#include <initializer_list>
#include <type_traits>

#include "posu_common.h"

namespace posu {
namespace {

// pixels in flight per thread in the partial passes (the sums do not depend on them: each thread
// adds its pixels in order).  The launches are ~256 blocks of 4 waves, one wave per SIMD, so the
// loads in flight per wave set the bandwidth.  4 and 8 are what runs and what was benchmarked:
// 8 or 2 in the backward pass lost in profiles/r04/bn_unroll_r4bn.txt, and 16 in both lost in
// round 6 (more registers, worse co-residency with the weight-gradient kernels sharing the CUs)
constexpr int kPartU1 = 4;  // the backward partial pass (z, gy and the mask per pixel)
constexpr int kPartU0 = 8;  // the forward statistics (z per pixel)
// partial-sum blocks per launch (target): 128 / 256 / 512 / 1024 measured 22.61 / 21.93 / 22.09 /
// 22.43 ms per training step
constexpr int kPartBlocks = 256;
// chunks in flight per thread in the segment-major apply passes (8 lost, bn_unroll_r4bn.txt)
constexpr int kSegU = 4;

constexpr int kMaxNB = 256;  // partial-sum blocks per segment

struct RedShape {
  int CPR, CB, PL, CG, NB, PPB;
};

RedShape red_shape(int Pseg, int C, int E, int nseg) {
  RedShape r;
  r.CPR = C / E;
  r.CB = std::min(r.CPR, 64);  // one wave of channel chunks per pixel row: wide layers get more blocks
  r.PL = 256 / r.CB;
  r.CG = (r.CPR + r.CB - 1) / r.CB;
  // <= 64 partial blocks per view of 4 (one load round per finalize lane)
  int nb = std::max(1, kPartBlocks / (r.CG * nseg));
  nb = std::min(nb, kMaxNB);
  nb = std::min(nb, std::max(1, Pseg / r.PL));
  // f64 partials of wide, short layers (layer4: 2048 channels x 2048 pixels per view) stay
  // below 1/8 of the input they reduce: at least 64 pixels per block
  nb = std::min(nb, std::max(1, Pseg / 64));
  r.NB = nb;
  r.PPB = (Pseg + nb - 1) / nb;
  return r;
}

// 16 B at p + off when `ok`, else zeros; a byte of m at i when `ok`, else 0.  Loaded from a valid
// address (`alt` when not ok) and selected by value: a select between *p and a local zero becomes
// a select of addresses, which puts the zero in scratch (the f16 / f32 kernels had 32 B of it)
template <typename T>
__device__ __forceinline__ uint4 ld16_if(bool ok, const T* p, const T* alt, size_t off) {
  const uint4 v = *reinterpret_cast<const uint4*>((ok ? p : alt) + off);
  return ok ? v : make_uint4(0, 0, 0, 0);
}
__device__ __forceinline__ unsigned ld8_if(bool ok, const uint8_t* m, const void* alt, size_t i) {
  const unsigned v = (ok ? m : static_cast<const uint8_t*>(alt))[i];
  return ok ? v : 0u;
}

// ---- the arithmetic of one 16-B chunk (E elements as f32), each piece written once.  The
// per-channel parameters are E consecutive floats, in registers or in global memory.

// out = a * b + c with one rounding per element, two elements per instruction (v_pk_fma_f32).
// Written on pairs: the compiler packs a run of scalar __builtin_fmaf calls only some of the time,
// and the backward passes are short of VALU slots.  out may be c.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int E>
__device__ __forceinline__ void fma_chunk(const float* a, const float* b, const float* c, float* out) {
#pragma unroll
  for (int e = 0; e < E; e += 2) {
    const f32x2 r = __builtin_elementwise_fma(f32x2{a[e], a[e + 1]}, f32x2{b[e], b[e + 1]}, f32x2{c[e], c[e + 1]});
    out[e] = r.x;
    out[e + 1] = r.y;
  }
}

// Vec<T>::pack of bn_dz's results.  Each product is made an f32 value of its own first: a multiply
// that feeds a conversion to f16 directly may be selected as v_fma_mixlo_f16, which rounds once, to
// f16 -- an ulp away, in some elements, from the f32 product rounded again, and chosen per copy of
// the code (one form of the segment-major backward had it in two elements of each chunk, the
// generic kernel in none).  The empty asm is the only fence the compiler offers for that.
template <typename T>
__device__ __forceinline__ uint4 pack_results(const float* v) {
  float r[Vec<T>::E];
#pragma unroll
  for (int e = 0; e < Vec<T>::E; e += 2) {
    f32x2 p = {v[e], v[e + 1]};  // in pairs, as the packed arithmetic leaves them
    asm("" : "+v"(p));
    r[e] = p.x;
    r[e + 1] = p.y;
  }
  return Vec<T>::pack(r);
}

// bit e = [v_e > 0]
template <typename T>
__device__ __forceinline__ uint8_t pos_bits(const float* v) {
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < Vec<T>::E; ++e) m |= (v[e] > 0.f ? 1u : 0u) << e;
  return static_cast<uint8_t>(m);
}

// y = act(z * scale + shift (+ r)) rounded to T, as the 16 B to store; r is read only when add_r
// (a flag, not a null r: a select between a register array and null would put the array in scratch).
// `bits` (optional): bit e = [y_e > 0] of the stored (rounded) values -- the mask the backward
// would read from y, at 1/16 of y's bytes
template <typename T>
__device__ __forceinline__ uint4 bn_act(const float* z, const float* sc, const float* sh, bool add_r, const float* r,
                                        bool relu, uint8_t* bits) {
  constexpr int E = Vec<T>::E;
  float v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    float t = __builtin_fmaf(z[e], sc[e], sh[e]);
    if (add_r) t += r[e];
    v[e] = relu ? fmaxf(t, 0.f) : t;
  }
  const uint4 o = Vec<T>::pack(v);
  if (bits) {
    Vec<T>::unpack(o, v);
    *bits = pos_bits<T>(v);
  }
  return o;
}

// g' = g * [y > 0] in place.  The ReLU mask comes from the forward's bit mask (one byte per chunk,
// bn_apply_mask), from y, or is recomputed from z (no residual: y > 0 <=> z * ks + kh > 0).  The
// y / z source's (wave-uniform) branches only decide which elements pass and g is selected once
// after them: branches that each rewrote g compiled to exec-masked code around every chunk
// (profiles/r07/bn_refactor_micro.txt, the backward lines 2-9 % slower).
enum Gate { kGateNone, kGateBits, kGateY, kGateZ };

__device__ __forceinline__ Gate gate_of(const void* ym, const void* y, const void* msc) {
  return ym ? kGateBits : y ? kGateY : msc ? kGateZ : kGateNone;
}

// BITS: the source is the bit mask, known when compiled -- the backward kernels run their loops in
// two copies, one for the bits (the training step's form; g selected straight from mq) and one for
// the other sources.  Copies of the loop, not kernels of their own: built as a kernel template
// parameter the bits' passes no longer batched their loads (bwd(mask,gres) 458 against 315 us,
// profiles/r07/bn_refactor_micro.txt).
template <typename T, bool BITS>
__device__ __forceinline__ void relu_gate(Gate src, float* g, unsigned mq, const uint4& yq, const float* z,
                                          const float* ks, const float* kh) {
  constexpr int E = Vec<T>::E;
  if constexpr (BITS) {
#pragma unroll
    for (int e = 0; e < E; ++e) g[e] = (mq >> e) & 1u ? g[e] : 0.f;
  } else {
    bool keep[E];  // element e passes
#pragma unroll
    for (int e = 0; e < E; ++e) keep[e] = true;
    if (src != kGateNone) {
      float yv[E];
      if (src == kGateY) Vec<T>::unpack(yq, yv);
      else fma_chunk<E>(z, ks, kh, yv);
#pragma unroll
      for (int e = 0; e < E; ++e) keep[e] = yv[e] > 0.f;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) g[e] = keep[e] ? g[e] : 0.f;
  }
}

__device__ __forceinline__ float bn_xhat(float z, float mu, float rd) { return (z - mu) * rd; }

// dz = gamma*rstd * (g' - mean(g') - xhat * mean(g' xhat)), over z in place; k1 / mg / mgx are
// the backward finalize's three coefficient rows
template <int E>
__device__ __forceinline__ void bn_dz(float* z, const float* g, const float* mu, const float* rd, const float* k1,
                                      const float* mg, const float* mgx) {
  float nxh[E], t[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    nxh[e] = -bn_xhat(z[e], mu[e], rd[e]);
    t[e] = g[e] - mg[e];
  }
  fma_chunk<E>(nxh, mgx, t, t);
#pragma unroll
  for (int e = 0; e < E; ++e) z[e] = k1[e] * t[e];
}

// one pixel of the partial pass: (a, b) += (z - K, (z - K)^2), and (a, b) += (g', g' * xhat)
template <int E>
__device__ __forceinline__ void acc_stats(float* a, float* b, const float* z, const float* kv) {
  float d[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    d[e] = z[e] - kv[e];
    a[e] += d[e];
  }
  fma_chunk<E>(d, d, b, b);
}
template <int E>
__device__ __forceinline__ void acc_grad(float* a, float* b, const float* g, const float* z, const float* mu,
                                         const float* rd) {
  float xh[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    a[e] += g[e];
    xh[e] = bn_xhat(z[e], mu[e], rd[e]);
  }
  fma_chunk<E>(g, xh, b, b);
}

// PyTorch's max-pool tie rule (pool.h max_pool2d `val > maxval || isnan(val)`): the first
// maximum in window scan order, a NaN taken.  am < 0: nothing taken yet
template <int E>
__device__ __forceinline__ void first_max(const float* v, int tap, float* m, int* am) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const bool take = am[e] < 0 || v[e] > m[e] || v[e] != v[e];
    m[e] = take ? v[e] : m[e];
    am[e] = take ? tap : am[e];
  }
}

// thread i of a pool launch over [n][rows][cols][chunks]: its chunk, column, row and image
template <typename I>
struct PoolPos {
  int ch, x, y;
  I n, pix;  // pix = (n * rows + y) * cols + x
};
template <typename I>
__device__ __forceinline__ PoolPos<I> pool_pos(I i, int chunks, int rows, int cols) {
  PoolPos<I> p;
  p.ch = static_cast<int>(i % chunks);
  p.pix = i / chunks;
  p.x = static_cast<int>(p.pix % cols);
  const I t = p.pix / cols;
  p.y = static_cast<int>(t % rows);
  p.n = t / rows;
  return p;
}

// MODE 0: (sum (z - K), sum (z - K)^2) -- forward statistics / channel sums; K = the
//         segment's first pixel when kout is non-null (shifted sums: a channel whose
//         mean is large against its spread keeps its variance in the f32 partials),
//         else 0.  Block 0 of each segment stores K to kout [nseg][C].
// MODE 1: (sum g', sum g' * xhat)     -- backward, g' = gy * [y > 0]: the ReLU mask from ym, y
//         or msc / msh (relu_gate); none of them: no ReLU
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_partial_kernel(const T* __restrict__ z, const T* __restrict__ gy,
                                                         const T* __restrict__ y, const float* __restrict__ msc,
                                                         const float* __restrict__ msh,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, int Pseg, int C,
                                                         RedShape rs, double* __restrict__ part,
                                                         float* __restrict__ kout, const uint8_t* __restrict__ ym) {
  constexpr int E = Vec<T>::E;
  __shared__ double red[2][256][E];
  const int tid = threadIdx.x;
  const int pl = tid / rs.CB, cb = tid - pl * rs.CB;
  const int ch = blockIdx.y * rs.CB + cb;
  const int seg = blockIdx.z, blk = blockIdx.x;
  const bool active = ch < rs.CPR;
  float a[E], b[E], mu[E], rd[E], ks[E], kh[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    a[e] = 0.f;
    b[e] = 0.f;
    mu[e] = 0.f;
    rd[e] = 0.f;
    ks[e] = 0.f;
    kh[e] = 0.f;
  }
  if (MODE == 1 && active) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      mu[e] = mean[seg * C + ch * E + e];
      rd[e] = rstd[seg * C + ch * E + e];
      if (msc) {
        ks[e] = msc[seg * C + ch * E + e];
        kh[e] = msh[seg * C + ch * E + e];
      }
    }
  }
  float kv[E];
#pragma unroll
  for (int e = 0; e < E; ++e) kv[e] = 0.f;
  if (MODE == 0 && kout && active) {
    Vec<T>::unpack(*reinterpret_cast<const uint4*>(z + static_cast<size_t>(seg) * Pseg * C + ch * E), kv);
    if (blk == 0 && pl == 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) kout[seg * C + ch * E + e] = kv[e];
    }
  }
  if (active) {
    const int pbeg = blk * rs.PPB, pend = min(Pseg, pbeg + rs.PPB);
    const size_t sbase = static_cast<size_t>(seg) * Pseg * C + ch * E;
    const Gate src = gate_of(ym, y, msc);
    // the pass in two copies: the bit mask as the ReLU source (BITS), or any other (relu_gate)
    auto pass = [&](auto bits) {
      constexpr bool BITS = decltype(bits)::value;
      // one pixel's contribution, accumulated in pixel order (the sums do not depend on U)
      auto acc = [&](const uint4& zq, const uint4& gq, const uint4& yq, unsigned mq) {
        float v[E];
        Vec<T>::unpack(zq, v);
        if constexpr (MODE == 0) {
          acc_stats<E>(a, b, v, kv);
        } else {
          float gv[E];
          Vec<T>::unpack(gq, gv);
          relu_gate<T, BITS>(src, gv, mq, yq, v, ks, kh);
          acc_grad<E>(a, b, gv, v, mu, rd);
        }
      };
      // U pixels per step with all their loads issued first (memory-level parallelism); the ReLU
      // source's loads behind wave-uniform branches (a y or mask load only when that is the source)
      constexpr int U = MODE == 0 ? kPartU0 : kPartU1;
      const uint4 zero = make_uint4(0, 0, 0, 0);
      const bool use_y = MODE == 1 && !BITS && y;
      constexpr bool use_m = BITS;
      int p = pbeg + pl;
      for (; p + (U - 1) * rs.PL < pend; p += U * rs.PL) {
        uint4 zq[U], gq[U], yq[U];
        unsigned mq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const size_t off = sbase + static_cast<size_t>(p + u * rs.PL) * C;
          zq[u] = *reinterpret_cast<const uint4*>(z + off);
          gq[u] = MODE == 1 ? *reinterpret_cast<const uint4*>(gy + off) : zero;
          yq[u] = zero;
          mq[u] = 0u;
        }
        if (use_y) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            yq[u] = *reinterpret_cast<const uint4*>(y + sbase + static_cast<size_t>(p + u * rs.PL) * C);
        } else if (use_m) {
#pragma unroll
          for (int u = 0; u < U; ++u) mq[u] = ym[(sbase + static_cast<size_t>(p + u * rs.PL) * C) / E];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc(zq[u], gq[u], yq[u], mq[u]);
      }
      for (; p < pend; p += rs.PL) {
        const size_t off = sbase + static_cast<size_t>(p) * C;
        acc(*reinterpret_cast<const uint4*>(z + off), MODE == 1 ? *reinterpret_cast<const uint4*>(gy + off) : zero,
            ld16_if(use_y, y, z, off), ld8_if(use_m, ym, z, off / E));
      }
    };
    if (MODE == 1 && ym) pass(std::true_type{});
    else pass(std::false_type{});
  }
  // the block's pixel lanes, paired in powers of two: sums and squares side by side through
  // 2 x [256][E] f64 (one quantity at a time through half the LDS was neutral in the step)
  double* dst = part + (static_cast<size_t>(seg) * rs.NB + blk) * 2 * C;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    red[0][tid][e] = a[e];
    red[1][tid][e] = b[e];
  }
  __syncthreads();
  for (int s = rs.PL / 2; s > 0; s >>= 1) {
    if (pl < s) {
      const int o = tid + s * rs.CB;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        red[0][tid][e] += red[0][o][e];
        red[1][tid][e] += red[1][o][e];
      }
    }
    __syncthreads();
  }
  if (pl == 0 && active) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      dst[ch * E + e] = red[0][tid][e];
      dst[C + ch * E + e] = red[1][tid][e];
    }
  }
}

// ---- finalize: the partials are a few hundred KiB, so this pass is latency-bound.  A block
// serves FC consecutive channels: lane ln of channel cl sums the partial blocks ln, ln + FL, ..
// (FIT of them per trip, for up to FSEG segments: every load of a trip issued before the first
// add), a wave's loads covering 4 blocks x 16 channels = 4 lines of 128 B; the FL lane sums meet
// in LDS and thread (k, cl) of wave 0 adds them in lane order (a fixed association), then does
// segment k's arithmetic -- the segments in parallel, not one lane's serial chain: 4.3 / 4.7 us
// per launch (statistics / backward).  The form that lost -- a half-wave per channel gathering 32
// scattered lines per load under per-segment branches, an xor butterfly, lane 0 doing the
// segments one after another: 9.8 / 8.3 us, 12 us in the training step's 112 launches -- is in
// profiles/r05/bn_finalize2_ab_r5bd.txt.
constexpr int FSEG = 4, FC = 16, FL = 16, FIT = 4;
constexpr int kFinLds = 2 * FSEG * FL * FC;  // doubles

// returns, in thread t < FSEG * FC (segment seg0 + t / FC, channel c0 + t % FC), the sums
// over the partial blocks; zeros elsewhere.  Every thread of the block calls it.
__device__ __forceinline__ void reduce_partials(const double* __restrict__ part, int seg0, int ns, int NB, int C,
                                                int c0, double* __restrict__ lds, double& s, double& q) {
  const int t = threadIdx.x, cl = t % FC, ln = t / FC;
  const int c = c0 + cl;
  const bool cv = c < C;
  double a[FSEG], b[FSEG];
#pragma unroll
  for (int k = 0; k < FSEG; ++k) a[k] = b[k] = 0.0;
  for (int base = 0; base < NB; base += FL * FIT) {
    double va[FSEG][FIT], vb[FSEG][FIT];
#pragma unroll
    for (int k = 0; k < FSEG; ++k)
#pragma unroll
      for (int j = 0; j < FIT; ++j) {
        const int blk = base + ln + FL * j;
        const bool ok = cv && k < ns && blk < NB;
        // a valid address either way, the value selected (no select of a load against a zero)
        const double* p = part + (ok ? static_cast<size_t>((seg0 + k) * NB + blk) * 2 * C + c : 0);
        const double x = p[0], y = p[ok ? C : 0];
        va[k][j] = ok ? x : 0.0;
        vb[k][j] = ok ? y : 0.0;
      }
#pragma unroll
    for (int k = 0; k < FSEG; ++k)
#pragma unroll
      for (int j = 0; j < FIT; ++j) {
        a[k] += va[k][j];
        b[k] += vb[k][j];
      }
  }
#pragma unroll
  for (int k = 0; k < FSEG; ++k) {
    lds[((0 * FSEG + k) * FL + ln) * FC + cl] = a[k];
    lds[((1 * FSEG + k) * FL + ln) * FC + cl] = b[k];
  }
  __syncthreads();
  s = q = 0.0;
  if (t < FSEG * FC) {
    const int k = t / FC;
#pragma unroll
    for (int l = 0; l < FL; ++l) {
      s += lds[((0 * FSEG + k) * FL + l) * FC + cl];
      q += lds[((1 * FSEG + k) * FL + l) * FC + cl];
    }
  }
  __syncthreads();  // lds is reused by the next call
}

__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(const double* __restrict__ part, int nseg, int NB,
                                                                int Pseg, int C, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps,
                                                                float momentum, const float* __restrict__ kshift,
                                                                float* __restrict__ running_mean,
                                                                float* __restrict__ running_var,
                                                                float* __restrict__ mean, float* __restrict__ rstd,
                                                                float* __restrict__ scale,
                                                                float* __restrict__ shift) {
  __shared__ double lds[kFinLds];
  __shared__ float mus[FSEG][FC], vus[FSEG][FC];
  const int t = threadIdx.x, k = t / FC, cl = t % FC;
  const int c0 = blockIdx.x * FC, c = c0 + cl;
  const bool mine = t < FSEG * FC && c < C;  // thread (segment k, channel c) of wave 0
  const double n = static_cast<double>(Pseg);
  const int cc = c < C ? c : 0;
  const float gm = gamma ? gamma[cc] : 1.f, bt = beta ? beta[cc] : 0.f;
  float rm = 0.f, rv = 0.f;
  if (t < FC && c < C) {
    rm = running_mean ? running_mean[c] : 0.f;
    rv = running_var ? running_var[c] : 0.f;
  }
  for (int seg0 = 0; seg0 < nseg; seg0 += FSEG) {
    const int ns = min(FSEG, nseg - seg0);
    const bool act = mine && k < ns;
    const int seg = seg0 + (act ? k : 0);
    const float ks = kshift[seg * C + cc];  // issued beside the partials
    double sum, sq;
    reduce_partials(part, seg0, ns, NB, C, c0, lds, sum, sq);
    if (act) {
      const double dm = sum / n;  // shifted by K = kshift[seg][c]
      const double mu = static_cast<double>(ks) + dm;
      const double var = fmax(sq / n - dm * dm, 0.0);
      const double r = 1.0 / sqrt(var + static_cast<double>(eps));
      mean[seg * C + c] = static_cast<float>(mu);
      rstd[seg * C + c] = static_cast<float>(r);
      scale[seg * C + c] = static_cast<float>(gm * r);
      shift[seg * C + c] = static_cast<float>(bt - mu * gm * r);
      mus[k][cl] = static_cast<float>(mu);
      vus[k][cl] = static_cast<float>(Pseg > 1 ? var * n / (n - 1.0) : var);
    }
    __syncthreads();
    if (t < FC && c < C)
      for (int j = 0; j < ns; ++j) {  // in segment order: running stats compose like V calls
        rm = (1.f - momentum) * rm + momentum * mus[j][t];
        rv = (1.f - momentum) * rv + momentum * vus[j][t];
      }
    __syncthreads();
  }
  if (t < FC && c < C) {
    if (running_mean) running_mean[c] = rm;
    if (running_var) running_var[c] = rv;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ part, int nseg, int NB,
                                                              int Pseg, int C, const float* __restrict__ gamma,
                                                              const float* __restrict__ rstd,
                                                              float* __restrict__ coef, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
  __shared__ double lds[kFinLds];
  __shared__ double sgs[FSEG][FC], sgxs[FSEG][FC];
  const int t = threadIdx.x, k = t / FC, cl = t % FC;
  const int c0 = blockIdx.x * FC, c = c0 + cl;
  const bool mine = t < FSEG * FC && c < C;
  const double n = static_cast<double>(Pseg);
  const int cc = c < C ? c : 0;
  const float gm = gamma ? gamma[cc] : 1.f;
  double tg = 0.0, tgx = 0.0;
  for (int seg0 = 0; seg0 < nseg; seg0 += FSEG) {
    const int ns = min(FSEG, nseg - seg0);
    const bool act = mine && k < ns;
    const int seg = seg0 + (act ? k : 0);
    const float rs = rstd[seg * C + cc];  // issued beside the partials
    double sg, sgx;
    reduce_partials(part, seg0, ns, NB, C, c0, lds, sg, sgx);
    if (act) {
      coef[(seg * 3 + 0) * C + c] = gm * rs;
      coef[(seg * 3 + 1) * C + c] = static_cast<float>(sg / n);
      coef[(seg * 3 + 2) * C + c] = static_cast<float>(sgx / n);
      sgs[k][cl] = sg;
      sgxs[k][cl] = sgx;
    }
    __syncthreads();
    if (t < FC && c < C)
      for (int j = 0; j < ns; ++j) {  // segment order
        tg += sgs[j][t];
        tgx += sgxs[j][t];
      }
    __syncthreads();
  }
  if (t < FC && c < C) {
    if (dgamma) dgamma[c] = static_cast<float>(tgx);
    if (dbeta) dbeta[c] = static_cast<float>(tg);
  }
}

__global__ __launch_bounds__(256) void channel_sum_finalize_kernel(const double* __restrict__ part, int NB, int C,
                                                                   float* __restrict__ out) {
  __shared__ double lds[kFinLds];
  const int t = threadIdx.x, c = blockIdx.x * FC + t % FC;
  double s, q;
  reduce_partials(part, 0, 1, NB, C, blockIdx.x * FC, lds, s, q);
  if (t < FC && c < C) out[c] = static_cast<float>(s);
}

// ---- apply: y = act(z * scale[seg] + shift[seg] (+ res)), one thread per 16-B chunk; mask
// (optional, ReLU only): one byte per chunk (bn_act).  The generic kernel reads the per-channel
// parameters from memory for every chunk; it serves C / E that does not divide 256 and parameter
// rows that are not 16-byte aligned.
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ z, int Pseg, int C,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const T* __restrict__ res,
                                                       int relu, T* __restrict__ y, long long total,
                                                       uint8_t* __restrict__ mask) {
  constexpr int E = Vec<T>::E;
  const int CPR = C / E;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
    const long long pix = i / CPR;
    const int c0 = static_cast<int>(i - pix * CPR) * E;
    const int seg = static_cast<int>(pix / Pseg);
    float v[E], r[E];
    Vec<T>::unpack(*reinterpret_cast<const uint4*>(z + i * E), v);
    if (res) Vec<T>::unpack(*reinterpret_cast<const uint4*>(res + i * E), r);
    *reinterpret_cast<uint4*>(y + i * E) =
        bn_act<T>(v, scale + seg * C + c0, shift + seg * C + c0, res != nullptr, r, relu, mask ? mask + i : nullptr);
  }
}

// Segment-major variants (C / E divides 256): blockIdx.y = segment, a thread's channel
// chunk never changes (the grid stride is a multiple of 256), so the per-channel
// parameters live in registers; U chunks per step with their loads issued first.
// The arithmetic per chunk is the generic kernels', through the same helpers.

// E consecutive per-channel f32 parameters as 16-B loads (E = 4 or 8; every parameter
// row starts at a multiple of 8 channels of a 16-B aligned allocation)
template <int E>
__device__ __forceinline__ void ldparams(const float* __restrict__ p, float* v) {
#pragma unroll
  for (int i = 0; i < E / 4; ++i) {
    const float4 q = reinterpret_cast<const float4*>(p)[i];
    v[4 * i] = q.x;
    v[4 * i + 1] = q.y;
    v[4 * i + 2] = q.z;
    v[4 * i + 3] = q.w;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_seg_kernel(const T* __restrict__ z, int Pseg, int C,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const T* __restrict__ res, int relu, T* __restrict__ y,
                                                           uint8_t* __restrict__ mask) {
  constexpr int E = Vec<T>::E, U = kSegU;
  const int CPR = C / E, seg = blockIdx.y;
  const int c0 = (threadIdx.x % CPR) * E;
  float sc[E], sh[E];
  ldparams<E>(scale + seg * C + c0, sc);
  ldparams<E>(shift + seg * C + c0, sh);
  const int n = Pseg * CPR, stride = gridDim.x * 256;
  const T* __restrict__ zs = z + static_cast<size_t>(seg) * Pseg * C;
  const T* __restrict__ rs = res ? res + static_cast<size_t>(seg) * Pseg * C : nullptr;
  T* __restrict__ ys = y + static_cast<size_t>(seg) * Pseg * C;
  uint8_t* __restrict__ ms = mask ? mask + static_cast<size_t>(seg) * Pseg * CPR : nullptr;
  auto one = [&](int i, const uint4& zq, const uint4& rq) {
    float v[E], r[E];
    Vec<T>::unpack(zq, v);
    if (rs) Vec<T>::unpack(rq, r);
    *reinterpret_cast<uint4*>(ys + static_cast<size_t>(i) * E) =
        bn_act<T>(v, sc, sh, rs != nullptr, r, relu, ms ? ms + i : nullptr);
  };
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; i + (U - 1) * stride < n; i += U * stride) {
    uint4 zq[U], rq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      zq[u] = *reinterpret_cast<const uint4*>(zs + static_cast<size_t>(i + u * stride) * E);
      rq[u] = ld16_if(rs != nullptr, rs, zs, static_cast<size_t>(i + u * stride) * E);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(i + u * stride, zq[u], rq[u]);
  }
  for (; i < n; i += stride)
    one(i, *reinterpret_cast<const uint4*>(zs + static_cast<size_t>(i) * E),
        ld16_if(rs != nullptr, rs, zs, static_cast<size_t>(i) * E));
}

// ---- backward apply: dz (bn_dz) from g' = gy * [y > 0] (relu_gate); gres (optional) = g',
// the gradient of the residual branch.  Segment-major first.  The generic kernel after it is held
// to 8 waves per SIMD (64 VGPRs; left alone the scheduler issues its ten parameter loads together,
// at 66).  bf16 and f16 sit at that limit: after a change to the helpers check this kernel's
// scratch in the code object (tools/isa_stats.py; zero today, profiles/r07/bn_refactor_regs.txt).
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_seg_kernel(const T* __restrict__ gy, const T* __restrict__ y,
                                                               const float* __restrict__ msc,
                                                               const float* __restrict__ msh,
                                                               const T* __restrict__ z, int Pseg, int C,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rstd,
                                                               const float* __restrict__ coef, T* __restrict__ dz,
                                                               T* __restrict__ gres, const uint8_t* __restrict__ ym) {
  constexpr int E = Vec<T>::E, U = kSegU;
  const int CPR = C / E, seg = blockIdx.y;
  const int c0 = (threadIdx.x % CPR) * E;
  float mu[E], rd[E], k1[E], mg[E], mgx[E], ks[E], kh[E];
  ldparams<E>(mean + seg * C + c0, mu);
  ldparams<E>(rstd + seg * C + c0, rd);
  ldparams<E>(coef + (seg * 3 + 0) * C + c0, k1);
  ldparams<E>(coef + (seg * 3 + 1) * C + c0, mg);
  ldparams<E>(coef + (seg * 3 + 2) * C + c0, mgx);
  if (msc) {
    ldparams<E>(msc + seg * C + c0, ks);
    ldparams<E>(msh + seg * C + c0, kh);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) ks[e] = kh[e] = 0.f;
  }
  const int n = Pseg * CPR, stride = gridDim.x * 256;
  const size_t sb = static_cast<size_t>(seg) * Pseg * C;
  const Gate src = gate_of(ym, y, msc);
  auto pass = [&](auto bits) {
    constexpr bool BITS = decltype(bits)::value;
    auto one = [&](int i, const uint4& gq, const uint4& zq, const uint4& yq, unsigned mq) {
      const size_t off = sb + static_cast<size_t>(i) * E;
      float g[E], v[E];
      Vec<T>::unpack(gq, g);
      Vec<T>::unpack(zq, v);
      relu_gate<T, BITS>(src, g, mq, yq, v, ks, kh);
      if (gres) *reinterpret_cast<uint4*>(gres + off) = Vec<T>::pack(g);
      bn_dz<E>(v, g, mu, rd, k1, mg, mgx);
      *reinterpret_cast<uint4*>(dz + off) = pack_results<T>(v);
    };
    int i = blockIdx.x * 256 + threadIdx.x;
    for (; i + (U - 1) * stride < n; i += U * stride) {
      uint4 gq[U], zq[U], yq[U];
      unsigned mq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t off = sb + static_cast<size_t>(i + u * stride) * E;
        gq[u] = *reinterpret_cast<const uint4*>(gy + off);
        zq[u] = *reinterpret_cast<const uint4*>(z + off);
        yq[u] = ld16_if(!BITS && y, y, z, off);
        mq[u] = ld8_if(BITS, ym, z, off / E);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) one(i + u * stride, gq[u], zq[u], yq[u], mq[u]);
    }
    for (; i < n; i += stride) {
      const size_t off = sb + static_cast<size_t>(i) * E;
      one(i, *reinterpret_cast<const uint4*>(gy + off), *reinterpret_cast<const uint4*>(z + off),
          ld16_if(!BITS && y, y, z, off), ld8_if(BITS, ym, z, off / E));
    }
  };
  if (ym) pass(std::true_type{});
  else pass(std::false_type{});
}

template <typename T>
__global__ __launch_bounds__(256, 8) void bn_bwd_apply_kernel(const T* __restrict__ gy, const T* __restrict__ y,
                                                           const float* __restrict__ msc,
                                                           const float* __restrict__ msh,
                                                           const T* __restrict__ z, int Pseg, int C,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ rstd,
                                                           const float* __restrict__ coef, T* __restrict__ dz,
                                                           T* __restrict__ gres, long long total,
                                                           const uint8_t* __restrict__ ym) {
  constexpr int E = Vec<T>::E;
  const int CPR = C / E;
  const Gate src = gate_of(ym, y, msc);
  auto pass = [&](auto bits) {
    constexpr bool BITS = decltype(bits)::value;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
      const long long pix = i / CPR;
      const int c0 = static_cast<int>(i - pix * CPR) * E;
      const int seg = static_cast<int>(pix / Pseg);
      const int pc = seg * C + c0;  // the chunk's place in a [nseg][C] parameter table
      float g[E], v[E];
      Vec<T>::unpack(*reinterpret_cast<const uint4*>(gy + i * E), g);
      Vec<T>::unpack(*reinterpret_cast<const uint4*>(z + i * E), v);
      relu_gate<T, BITS>(src, g, ld8_if(BITS, ym, z, i), ld16_if(!BITS && y, y, z, i * E), v,
                         src == kGateZ ? msc + pc : nullptr, src == kGateZ ? msh + pc : nullptr);
      if (gres) *reinterpret_cast<uint4*>(gres + i * E) = Vec<T>::pack(g);
      bn_dz<E>(v, g, mean + pc, rstd + pc, coef + (seg * 3 + 0) * C + c0, coef + (seg * 3 + 1) * C + c0,
               coef + (seg * 3 + 2) * C + c0);
      *reinterpret_cast<uint4*>(dz + i * E) = pack_results<T>(v);
    }
  };
  if (ym) pass(std::true_type{});
  else pass(std::false_type{});
}

// blocks per segment of a segment-major launch: at least 16 chunks per thread (the
// per-channel parameters are loaded once per thread), at most about 1024 blocks in all
inline int seg_blocks(int Pseg, int C, int E, int nseg) {
  const long long chunks = static_cast<long long>(Pseg) * (C / E);
  const long long need = (chunks + 256LL * 16 - 1) / (256LL * 16);
  const long long cap = std::max(1, 1024 / nseg);
  return static_cast<int>(std::max(1LL, std::min(need, cap)));
}

inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

inline bool seg_major(int C, int E, int nseg, int Pseg, std::initializer_list<const void*> params) {
  for (const void* p : params)
    if (p && !aligned16(p)) return false;
  const int cpr = C / E;
  // the loops index chunks in int: i + (U - 1) * stride and i + U * stride must stay below
  // 2^31 for the largest i < Pseg * cpr (stride <= 1024 blocks * 256 threads)
  const long long n = static_cast<long long>(Pseg) * cpr;
  return cpr > 0 && 256 % cpr == 0 && nseg <= 65535 && n + static_cast<long long>(kSegU) * 1024 * 256 < (1LL << 31);
}

// ---- max-pool 3x3 / s2 / p1 backward (the tie rule: first_max).
// pass 1: argmax tap (0..8) per output element; pass 2: every input element gathers
// the gradients of the (at most 2 x 2) windows whose argmax it is -- no atomics.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_argmax_kernel(const T* __restrict__ x, int N, int H, int W, int C,
                                                             int Ho, int Wo, uint8_t* __restrict__ idx) {
  constexpr int E = Vec<T>::E;
  const int chunks = C / E;
  const long long total = static_cast<long long>(N) * Ho * Wo * chunks;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
    const PoolPos<long long> o = pool_pos(i, chunks, Ho, Wo);
    float m[E];
    int am[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      m[e] = 0.f;
      am[e] = -1;
    }
#pragma unroll 1  // one tap's load and compare in the loop, as in the fused stem pool
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - 3 * dy;
      const int iy = o.y * 2 - 1 + dy, ix = o.x * 2 - 1 + dx;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      float v[E];
      Vec<T>::unpack(*reinterpret_cast<const uint4*>(x + ((o.n * H + iy) * W + ix) * C + o.ch * E), v);
      first_max<E>(v, tap, m, am);
    }
    uint8_t* dst = idx + o.pix * C + o.ch * E;
#pragma unroll
    for (int e = 0; e < E; ++e) dst[e] = static_cast<uint8_t>(am[e]);
  }
}

// pass 2: a thread per 2x2 input block (rows 2a, 2a+1, columns 2b, 2b+1) and 16-B channel chunk.
// Input row 2a lies in window row a only (tap row 1), row 2a+1 in window rows a (tap row 2) and
// a+1 (tap row 0), and likewise for columns, so the block's four outputs need exactly the windows
// (a | a+1) x (b | b+1): four gradient / tap loads per four stores, no data-dependent loop and
// 32-bit index math, the windows added in increasing (oy, ox) order: 95 us for the training
// stem's 268 MB at 128 frames.  A thread per input chunk looping over its windows (2.25 window
// loads per chunk, 64-bit divisions) took 193 us: profiles/r05/pool_bwd2_ab_r5bj.txt.  The
// entry points refuse a launch of 2^31 - 256 blocks of 2x2 or more.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const uint8_t* __restrict__ idx, const T* __restrict__ gy,
                                                          int N, int H, int W, int C, int Ho, int Wo,
                                                          T* __restrict__ gx) {
  constexpr int E = Vec<T>::E;
  const int chunks = C / E, Hq = (H + 1) / 2, Wq = (W + 1) / 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * Hq * Wq * chunks) return;
  const PoolPos<int> q = pool_pos(i, chunks, Hq, Wq);
  const int ch = q.ch, b = q.x, a = q.y, n = q.n;
  float g[2][2][E];
  unsigned long long tv[2][2];
#pragma unroll
  for (int wy = 0; wy < 2; ++wy)
#pragma unroll
    for (int wx = 0; wx < 2; ++wx) {
      const bool ok = a + wy < Ho && b + wx < Wo;
      // a valid address either way, the value selected (an absent window matches no tap)
      const size_t o = ok ? ((static_cast<size_t>(n) * Ho + a + wy) * Wo + b + wx) * C + ch * E : 0;
      const uint4 gq = *reinterpret_cast<const uint4*>(gy + o);
      unsigned long long t;
      if constexpr (E == 8) t = *reinterpret_cast<const unsigned long long*>(idx + o);
      else t = *reinterpret_cast<const unsigned*>(idx + o);
      Vec<T>::unpack(ok ? gq : make_uint4(0, 0, 0, 0), g[wy][wx]);
      tv[wy][wx] = ok ? t : ~0ull;
    }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int iy = 2 * a + r, ix = 2 * b + c;
      if (iy >= H || ix >= W) continue;
      float acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
      for (int wy = 0; wy < 2; ++wy) {
        if (r == 0 && wy == 1) continue;   // even row: window row a only (tap row 1)
        const unsigned ty = r == 0 ? 1u : (wy == 0 ? 2u : 0u);
#pragma unroll
        for (int wx = 0; wx < 2; ++wx) {
          if (c == 0 && wx == 1) continue;
          const unsigned tap = ty * 3 + (c == 0 ? 1u : (wx == 0 ? 2u : 0u));
#pragma unroll
          for (int e = 0; e < E; ++e)
            if (((tv[wy][wx] >> (8 * e)) & 0xffu) == tap) acc[e] += g[wy][wx][e];
        }
      }
      *reinterpret_cast<uint4*>(gx + ((static_cast<size_t>(n) * H + iy) * W + ix) * C + ch * E) = Vec<T>::pack(acc);
    }
}

// Training stem (round 5): a = relu(z * scale[seg] + shift[seg]) rounded to the dtype (bn_act),
// its 3x3 / s2 / p1 max-pool (maxpool_kernel's fmaxf over the window) and the argmax tap per
// output element (first_max) in one pass over z, without writing a: the backward takes the taps
// (maxpool_bwd_kernel) and its ReLU mask from z.  Replaces bn_apply + maxpool + the backward's
// argmax pass (1.17 GB -> 0.37 GB per step at the training stem's 128 x 128 x 128 x 64).
template <typename T>
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const T* __restrict__ z, int N, int nimg, int H, int W,
                                                              int C, int Ho, int Wo, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, T* __restrict__ y,
                                                              uint8_t* __restrict__ idx) {
  constexpr int E = Vec<T>::E;
  const int chunks = C / E;
  const long long total = static_cast<long long>(N) * Ho * Wo * chunks;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
    const PoolPos<long long> o = pool_pos(i, chunks, Ho, Wo);
    const int seg = static_cast<int>(o.n / nimg);
    float sc[E], sh[E], m[E], bm[E];
    int am[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      sc[e] = scale[seg * C + o.ch * E + e];
      sh[e] = shift[seg * C + o.ch * E + e];
      m[e] = -INFINITY;
      bm[e] = 0.f;
      am[e] = -1;
    }
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - 3 * dy;
      const int iy = o.y * 2 - 1 + dy, ix = o.x * 2 - 1 + dx;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      float v[E];
      Vec<T>::unpack(*reinterpret_cast<const uint4*>(z + ((o.n * H + iy) * W + ix) * C + o.ch * E), v);
      Vec<T>::unpack(bn_act<T>(v, sc, sh, false, nullptr, true, nullptr), v);  // the activation as bn_apply stores it
#pragma unroll
      for (int e = 0; e < E; ++e) m[e] = fmaxf(m[e], v[e]);
      first_max<E>(v, tap, bm, am);
    }
    *reinterpret_cast<uint4*>(y + o.pix * C + o.ch * E) = Vec<T>::pack(m);
    uint8_t* dst = idx + o.pix * C + o.ch * E;
#pragma unroll
    for (int e = 0; e < E; ++e) dst[e] = static_cast<uint8_t>(am[e]);
  }
}

inline int grid_for(long long total) {
  long long g = (total + 255) / 256;
  return static_cast<int>(g < 8192 ? (g > 0 ? g : 1) : 8192);
}

int chunk_elems(int dtype) { return dtype == POSU_F32 ? 4 : 8; }

// the block reduction pairs pixel lanes in powers of two
bool reducible(int C, int dtype) {
  const int cpr = C / chunk_elems(dtype);
  return cpr >= 256 ? cpr % 256 == 0 : ilog2(cpr) >= 0;
}

// threads of a maxpool_bwd_kernel launch (one per 2x2 input block and chunk), and whether its
// 32-bit index math holds them
long long pool_quads(int N, int H, int W, int C, int E) {
  return static_cast<long long>(N) * ((H + 1) / 2) * ((W + 1) / 2) * (C / E);
}
bool pool_bwd_fits(int dtype, int N, int H, int W, int C) {
  return pool_quads(N, H, W, C, chunk_elems(dtype)) < (1LL << 31) - 256;
}

template <typename T>
void pool_bwd_launch(const uint8_t* idx, const T* gy, int N, int H, int W, int C, int Ho, int Wo, T* gx,
                     hipStream_t s) {
  const long long quads = pool_quads(N, H, W, C, Vec<T>::E);
  hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(static_cast<unsigned>((quads + 255) / 256)), dim3(256), 0, s, idx,
                     gy, N, H, W, C, Ho, Wo, gx);
}

long long partial_bytes(int nseg, int C) { return static_cast<long long>(nseg) * kMaxNB * 2 * C * 8; }

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" long long posu_bn_workspace(int nseg, int C) {
  return partial_bytes(nseg, C) + static_cast<long long>(nseg) * 3 * C * 4;
}

extern "C" int posu_bn_train_fwd(int dtype, const void* z, int nseg, int Pseg, int C, const float* gamma,
                                 const float* beta, float eps, float momentum, float* running_mean,
                                 float* running_var, float* mean, float* rstd, float* scale, float* shift,
                                 void* workspace, long long workspace_bytes, void* stream) {
  POSU_REQUIRE(z && mean && rstd && scale && shift && workspace, "posu_bn_train_fwd: null pointer");
  POSU_REQUIRE(nseg > 0 && Pseg > 0 && C > 0 && C % chunk_elems(dtype) == 0 && reducible(C, dtype),
               "posu_bn_train_fwd: bad shape (C / chunk must be a power of two or a multiple of 256)");
  POSU_REQUIRE(workspace_bytes >= posu_bn_workspace(nseg, C), "posu_bn_train_fwd: workspace too small");
  hipStream_t s = as_stream(stream);
  double* part = static_cast<double*>(workspace);
  // the per-segment shifts K live where the backward keeps its coefficients
  float* kshift = reinterpret_cast<float*>(static_cast<char*>(workspace) + partial_bytes(nseg, C));
  const RedShape rs = red_shape(Pseg, C, chunk_elems(dtype), nseg);
  const bool ok = with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((bn_partial_kernel<T, 0>), dim3(rs.NB, rs.CG, nseg), dim3(256), 0, s,
                       static_cast<const T*>(z), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, Pseg, C, rs,
                       part, kshift, nullptr);
  });
  POSU_REQUIRE(ok, "posu_bn_train_fwd: unsupported dtype");
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((C + FC - 1) / FC), dim3(256), 0, s, part, nseg, rs.NB, Pseg, C,
                     gamma, beta, eps, momentum, kshift, running_mean, running_var, mean, rstd, scale, shift);
  return check_launch("posu_bn_train_fwd");
}

namespace {
int bn_apply_impl(const char* name, int dtype, const void* z, int nseg, int Pseg, int C, const float* scale,
                  const float* shift, const void* residual, int relu, void* y, void* mask, void* stream) {
  const std::string what = name;
  POSU_REQUIRE(z && scale && shift && y, what + ": null pointer");
  POSU_REQUIRE(nseg > 0 && Pseg > 0 && C > 0 && C % chunk_elems(dtype) == 0, what + ": bad shape");
  hipStream_t s = as_stream(stream);
  const long long total = static_cast<long long>(nseg) * Pseg * C / chunk_elems(dtype);
  const int E = chunk_elems(dtype);
  uint8_t* mk = static_cast<uint8_t*>(mask);
  const bool ok = with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (seg_major(C, E, nseg, Pseg, {scale, shift})) {
      hipLaunchKernelGGL(bn_apply_seg_kernel<T>, dim3(seg_blocks(Pseg, C, E, nseg), nseg), dim3(256), 0, s,
                         static_cast<const T*>(z), Pseg, C, scale, shift, static_cast<const T*>(residual), relu,
                         static_cast<T*>(y), mk);
      return;
    }
    hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, static_cast<const T*>(z), Pseg,
                       C, scale, shift, static_cast<const T*>(residual), relu, static_cast<T*>(y), total, mk);
  });
  POSU_REQUIRE(ok, what + ": unsupported dtype");
  return check_launch(name);
}

int bn_bwd_impl(const char* name, int dtype, const void* gy, const void* y, const void* ymask,
                const float* relu_scale, const float* relu_shift, const void* z, int nseg, int Pseg, int C,
                const float* mean, const float* rstd, const float* gamma, float* dgamma, float* dbeta, void* dz,
                void* gres, void* workspace, long long workspace_bytes, void* stream) {
  const std::string what = name;
  POSU_REQUIRE(gy && z && mean && rstd && dz && workspace, what + ": null pointer");
  POSU_REQUIRE(nseg > 0 && Pseg > 0 && C > 0 && C % chunk_elems(dtype) == 0 && reducible(C, dtype),
               what + ": bad shape (C / chunk must be a power of two or a multiple of 256)");
  POSU_REQUIRE(workspace_bytes >= posu_bn_workspace(nseg, C), what + ": workspace too small");
  hipStream_t s = as_stream(stream);
  double* part = static_cast<double*>(workspace);
  float* coef = reinterpret_cast<float*>(static_cast<char*>(workspace) + partial_bytes(nseg, C));
  const RedShape rs = red_shape(Pseg, C, chunk_elems(dtype), nseg);
  const long long total = static_cast<long long>(nseg) * Pseg * C / chunk_elems(dtype);
  const uint8_t* ym = static_cast<const uint8_t*>(ymask);
  bool ok = with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((bn_partial_kernel<T, 1>), dim3(rs.NB, rs.CG, nseg), dim3(256), 0, s,
                       static_cast<const T*>(z), static_cast<const T*>(gy), static_cast<const T*>(y), relu_scale,
                       relu_shift, mean, rstd, Pseg, C, rs, part, nullptr, ym);
  });
  POSU_REQUIRE(ok, what + ": unsupported dtype");
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FC - 1) / FC), dim3(256), 0, s, part, nseg, rs.NB, Pseg, C,
                     gamma, rstd, coef, dgamma, dbeta);
  with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    const int E = chunk_elems(dtype);
    if (seg_major(C, E, nseg, Pseg, {mean, rstd, coef, relu_scale, relu_shift})) {
      hipLaunchKernelGGL(bn_bwd_apply_seg_kernel<T>, dim3(seg_blocks(Pseg, C, E, nseg), nseg), dim3(256), 0, s,
                         static_cast<const T*>(gy), static_cast<const T*>(y), relu_scale, relu_shift,
                         static_cast<const T*>(z), Pseg, C, mean, rstd, coef, static_cast<T*>(dz),
                         static_cast<T*>(gres), ym);
      return;
    }
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, static_cast<const T*>(gy),
                       static_cast<const T*>(y), relu_scale, relu_shift, static_cast<const T*>(z), Pseg, C, mean, rstd,
                       coef, static_cast<T*>(dz), static_cast<T*>(gres), total, ym);
  });
  return check_launch(name);
}
}  // namespace

extern "C" int posu_bn_apply(int dtype, const void* z, int nseg, int Pseg, int C, const float* scale,
                             const float* shift, const void* residual, int relu, void* y, void* stream) {
  return bn_apply_impl("posu_bn_apply", dtype, z, nseg, Pseg, C, scale, shift, residual, relu, y, nullptr, stream);
}

extern "C" int posu_bn_apply_mask(int dtype, const void* z, int nseg, int Pseg, int C, const float* scale,
                                  const float* shift, const void* residual, void* y, void* mask, void* stream) {
  POSU_REQUIRE(mask, "posu_bn_apply_mask: null pointer (mask)");
  POSU_REQUIRE(mask != y && mask != z && mask != residual, "posu_bn_apply_mask: the mask must not alias a tensor");
  return bn_apply_impl("posu_bn_apply_mask", dtype, z, nseg, Pseg, C, scale, shift, residual, 1, y, mask, stream);
}

extern "C" int posu_bn_train_bwd(int dtype, const void* gy, const void* y, const float* relu_scale,
                                 const float* relu_shift, const void* z, int nseg, int Pseg, int C,
                                 const float* mean, const float* rstd, const float* gamma, float* dgamma,
                                 float* dbeta, void* dz, void* gres, void* workspace, long long workspace_bytes,
                                 void* stream) {
  return bn_bwd_impl("posu_bn_train_bwd", dtype, gy, y, nullptr, relu_scale, relu_shift, z, nseg, Pseg, C, mean,
                     rstd, gamma, dgamma, dbeta, dz, gres, workspace, workspace_bytes, stream);
}

extern "C" int posu_bn_train_bwd_mask(int dtype, const void* gy, const void* mask, const void* z, int nseg, int Pseg,
                                      int C, const float* mean, const float* rstd, const float* gamma, float* dgamma,
                                      float* dbeta, void* dz, void* gres, void* workspace, long long workspace_bytes,
                                      void* stream) {
  POSU_REQUIRE(mask, "posu_bn_train_bwd_mask: null pointer (mask)");
  return bn_bwd_impl("posu_bn_train_bwd_mask", dtype, gy, nullptr, mask, nullptr, nullptr, z, nseg, Pseg, C, mean,
                     rstd, gamma, dgamma, dbeta, dz, gres, workspace, workspace_bytes, stream);
}

extern "C" int posu_channel_sum(int dtype, const void* x, int P, int C, float* out, void* workspace,
                                long long workspace_bytes, void* stream) {
  POSU_REQUIRE(x && out && workspace, "posu_channel_sum: null pointer");
  POSU_REQUIRE(P > 0 && C > 0 && C % chunk_elems(dtype) == 0 && reducible(C, dtype),
               "posu_channel_sum: bad shape (C / chunk must be a power of two or a multiple of 256)");
  POSU_REQUIRE(workspace_bytes >= posu_bn_workspace(1, C), "posu_channel_sum: workspace too small");
  hipStream_t s = as_stream(stream);
  double* part = static_cast<double*>(workspace);
  const RedShape rs = red_shape(P, C, chunk_elems(dtype), 1);
  const bool ok = with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((bn_partial_kernel<T, 0>), dim3(rs.NB, rs.CG, 1), dim3(256), 0, s, static_cast<const T*>(x),
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, P, C, rs, part, nullptr, nullptr);
  });
  POSU_REQUIRE(ok, "posu_channel_sum: unsupported dtype");
  hipLaunchKernelGGL(channel_sum_finalize_kernel, dim3((C + FC - 1) / FC), dim3(256), 0, s, part, rs.NB, C, out);
  return check_launch("posu_channel_sum");
}

extern "C" long long posu_maxpool3x3s2_bwd_workspace(int N, int H, int W, int C) {
  const long long Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  return N * Ho * Wo * C;
}

extern "C" int posu_maxpool3x3s2_bwd(int dtype, const void* x, int N, int H, int W, int C, const void* gy, void* gx,
                                     void* workspace, long long workspace_bytes, void* stream) {
  POSU_REQUIRE(x && gy && gx && workspace, "posu_maxpool3x3s2_bwd: null pointer");
  POSU_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % chunk_elems(dtype) == 0, "posu_maxpool3x3s2_bwd: bad shape");
  POSU_REQUIRE(workspace_bytes >= posu_maxpool3x3s2_bwd_workspace(N, H, W, C),
               "posu_maxpool3x3s2_bwd: workspace too small");
  POSU_REQUIRE(pool_bwd_fits(dtype, N, H, W, C), "posu_maxpool3x3s2_bwd: shape too large");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipStream_t s = as_stream(stream);
  uint8_t* idx = static_cast<uint8_t*>(workspace);
  const int E = chunk_elems(dtype);
  const bool ok = with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(maxpool_argmax_kernel<T>, dim3(grid_for(static_cast<long long>(N) * Ho * Wo * C / E)),
                       dim3(256), 0, s, static_cast<const T*>(x), N, H, W, C, Ho, Wo, idx);
    pool_bwd_launch<T>(idx, static_cast<const T*>(gy), N, H, W, C, Ho, Wo, static_cast<T*>(gx), s);
  });
  POSU_REQUIRE(ok, "posu_maxpool3x3s2_bwd: unsupported dtype");
  return check_launch("posu_maxpool3x3s2_bwd");
}

extern "C" int posu_bn_relu_maxpool3x3s2_fwd(int dtype, const void* z, int nseg, int N, int H, int W, int C,
                                             const float* scale, const float* shift, void* y, void* idx,
                                             void* stream) {
  POSU_REQUIRE(z && scale && shift && y && idx, "posu_bn_relu_maxpool3x3s2_fwd: null pointer");
  POSU_REQUIRE(nseg > 0 && N > 0 && N % nseg == 0 && H > 0 && W > 0 && C > 0 && C % chunk_elems(dtype) == 0,
               "posu_bn_relu_maxpool3x3s2_fwd: bad shape (N a multiple of nseg, C of the 16-B chunk)");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipStream_t s = as_stream(stream);
  const int E = chunk_elems(dtype);
  const bool ok = with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(bn_relu_maxpool_kernel<T>, dim3(grid_for(static_cast<long long>(N) * Ho * Wo * C / E)),
                       dim3(256), 0, s, static_cast<const T*>(z), N, N / nseg, H, W, C, Ho, Wo, scale, shift,
                       static_cast<T*>(y), static_cast<uint8_t*>(idx));
  });
  POSU_REQUIRE(ok, "posu_bn_relu_maxpool3x3s2_fwd: unsupported dtype");
  return check_launch("posu_bn_relu_maxpool3x3s2_fwd");
}

extern "C" int posu_maxpool3x3s2_bwd_idx(int dtype, const void* idx, const void* gy, int N, int H, int W, int C,
                                         void* gx, void* stream) {
  POSU_REQUIRE(idx && gy && gx, "posu_maxpool3x3s2_bwd_idx: null pointer");
  POSU_REQUIRE((reinterpret_cast<size_t>(idx) & 7) == 0, "posu_maxpool3x3s2_bwd_idx: idx must be 8-byte aligned");
  POSU_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % chunk_elems(dtype) == 0, "posu_maxpool3x3s2_bwd_idx: bad shape");
  POSU_REQUIRE(pool_bwd_fits(dtype, N, H, W, C), "posu_maxpool3x3s2_bwd_idx: shape too large");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipStream_t s = as_stream(stream);
  const bool ok = with_storage(dtype, [&](auto tag) {
    using T = decltype(tag);
    pool_bwd_launch<T>(static_cast<const uint8_t*>(idx), static_cast<const T*>(gy), N, H, W, C, Ho, Wo,
                       static_cast<T*>(gx), s);
  });
  POSU_REQUIRE(ok, "posu_maxpool3x3s2_bwd_idx: unsupported dtype");
  return check_launch("posu_maxpool3x3s2_bwd_idx");
}
