// Adam update of the training step (BASELINE configs[3]; the reference's optimizer is
// torch.optim.Adam, utils/utils.py:79-83, stepped by core/function.py:366) over every parameter
// tensor of the network in a few launches: per element
//   g' = g (+ weight_decay * p)
//   m  = beta1 m + (1 - beta1) g'
//   v  = beta2 v + (1 - beta2) g'^2
//   p  = p - step_size * m / (sqrt(v) / sqrt(bc2) + eps),   step_size = lr / bc1,
//   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (the host computes both in double),
// the order of torch's Adam, in f32 (torch's kernels carry some of the products in double: the
// results agree within f32 rounding, not bit for bit).  HBM-bound: 28 B per element (p, g, m, v
// read; p, m, v written).  torch's fused multi-tensor Adam splits the step into launches of at
// most 320 chunks (~1.3 blocks per CU, 3.1 TB/s on the benched step); here every launch takes up
// to kAdamTensors tensors by value (kernel arguments, nothing to stage in device memory), one
// 2048-element chunk per block, a block finding its tensor by a scan of the launch's block
// offsets.
//
// fp16 training adds three passes on the same launch table (second half of this file): the
// gradients' overflow flag / sum of squares / in-place unscale (posu_grad_stats), Adam with the
// step count, the loss scale and the overflow flag in device memory (posu_adam_step_dev) and the
// loss scale's update (posu_loss_scale_update).
#include <cmath>

#include "posu_common.h"
#include "../../include/posu.h"

namespace posu {
namespace {

constexpr int kAdamTensors = 64;   // 64 x 40 B tensor records + offsets + scalars: 3.1 KB of kernel arguments (< 4 KB)
constexpr int kAdamThreads = 256, kAdamVec = 2;   // 2 float4 per thread: 2048 elements per block
constexpr int kAdamChunk = kAdamThreads * 4 * kAdamVec;

struct AdamLaunch {
  posu_adam_tensor t[kAdamTensors];
  long long blk0[kAdamTensors + 1];   // first block of tensor i; blk0[nt] = the launch's blocks
  int nt;
  float step_size, inv_bc2s, beta1, beta2, omb1, omb2, eps, wd;
};

template <typename A>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const A& a) {
  // the fused multiply-adds are spelled out (they are the ones the compiler's contraction chose for
  // adam_kernel), so that every kernel built on this function rounds alike: left to the
  // contraction, adam_dev_kernel's float4 path fused the other product and differed in the last bit
  if (a.wd != 0.f) g = __builtin_fmaf(a.wd, p, g);
  m = __builtin_fmaf(a.beta1, m, a.omb1 * g);
  v = __builtin_fmaf(a.beta2, v, a.omb2 * g * g);
  const float denom = __builtin_fmaf(sqrtf(v), a.inv_bc2s, a.eps);
  p -= a.step_size * m / denom;
}

// One block's 2048-element chunk [e0, e1) of tensor t (posu_adam_tensor or posu_adam_dev_tensor);
// Scaled: the gradient is multiplied by gmul first (the loss scale's reciprocal times the clip).
template <bool Scaled, typename T, typename A>
__device__ __forceinline__ void adam_chunk(const T& t, long long e0, long long e1, const A& a, float gmul) {
  const bool vec = ((reinterpret_cast<size_t>(t.p) | reinterpret_cast<size_t>(t.g) | reinterpret_cast<size_t>(t.m) |
                     reinterpret_cast<size_t>(t.v)) & 15) == 0;
  if (vec && e1 - e0 == kAdamChunk) {
    float4 p4[kAdamVec], g4[kAdamVec], m4[kAdamVec], v4[kAdamVec];
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u) {
      const long long i = e0 / 4 + u * kAdamThreads + threadIdx.x;
      p4[u] = reinterpret_cast<const float4*>(t.p)[i];
      g4[u] = reinterpret_cast<const float4*>(t.g)[i];
      m4[u] = reinterpret_cast<const float4*>(t.m)[i];
      v4[u] = reinterpret_cast<const float4*>(t.v)[i];
      if (Scaled) {
        g4[u].x *= gmul;
        g4[u].y *= gmul;
        g4[u].z *= gmul;
        g4[u].w *= gmul;
      }
    }
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u) {
      adam_one(p4[u].x, g4[u].x, m4[u].x, v4[u].x, a);
      adam_one(p4[u].y, g4[u].y, m4[u].y, v4[u].y, a);
      adam_one(p4[u].z, g4[u].z, m4[u].z, v4[u].z, a);
      adam_one(p4[u].w, g4[u].w, m4[u].w, v4[u].w, a);
      const long long i = e0 / 4 + u * kAdamThreads + threadIdx.x;
      reinterpret_cast<float4*>(t.p)[i] = p4[u];
      reinterpret_cast<float4*>(t.m)[i] = m4[u];
      reinterpret_cast<float4*>(t.v)[i] = v4[u];
    }
    return;
  }
  for (long long i = e0 + threadIdx.x; i < e1; i += kAdamThreads) {   // ragged / unaligned tail
    float p = t.p[i], m = t.m[i], v = t.v[i];
    adam_one(p, Scaled ? t.g[i] * gmul : t.g[i], m, v, a);
    t.p[i] = p;
    t.m[i] = m;
    t.v[i] = v;
  }
}

// the tensor of block b in a launch's block offsets (uniform scan over <= 64 offsets; tensors
// without blocks are passed over)
__device__ __forceinline__ int tensor_of_block(const long long* blk0, int nt, long long b) {
  int ti = 0;
  while (ti + 1 < nt && blk0[ti + 1] <= b) ++ti;
  return ti;
}

__global__ __launch_bounds__(kAdamThreads) void adam_kernel(const AdamLaunch a) {
  const long long b = blockIdx.x;
  const int ti = tensor_of_block(a.blk0, a.nt, b);
  const posu_adam_tensor& t = a.t[ti];
  const long long e0 = (b - a.blk0[ti]) * kAdamChunk;
  adam_chunk<false>(t, e0, min(t.n, e0 + kAdamChunk), a, 1.f);
}

// ---------------------------------------------------------------------------------------------
// fp16 training: the loss-scaling passes.  All three are enqueue-only and read what decides the
// step (found_inf, the scale, the step counters) from device memory, so a training loop neither
// synchronises nor leaves a captured graph.

// Adam with the step on the device (posu_adam_step_dev): 64 x 48 B records + 65 offsets + the
// scalars and pointers below = 3.7 KB of kernel arguments (< 4 KB, as above).
struct AdamDevLaunch {
  posu_adam_dev_tensor t[kAdamTensors];
  long long blk0[kAdamTensors + 1];
  int nt;
  float eps, wd, max_norm;   // max_norm <= 0: no clipping
  double lr, beta1, beta2;
  const float* found_inf;
  const float* scale;
  const double* sumsq;
};
static_assert(sizeof(AdamDevLaunch) < 4096, "AdamDevLaunch must fit the kernel-argument budget");

struct AdamCoef {
  float step_size, inv_bc2s, beta1, beta2, omb1, omb2, eps, wd;
};

// step += 1 for every tensor of the launch unless the gradients overflowed; one thread per tensor
__global__ __launch_bounds__(kAdamTensors) void adam_dev_prologue(const AdamDevLaunch a) {
  if (a.found_inf && *a.found_inf != 0.f) return;
  if (static_cast<int>(threadIdx.x) < a.nt) *a.t[threadIdx.x].step += 1.f;
}

__global__ __launch_bounds__(kAdamThreads) void adam_dev_kernel(const AdamDevLaunch a) {
  if (a.found_inf && *a.found_inf != 0.f) return;   // overflowed step: no store at all
  const long long b = blockIdx.x;
  const int ti = tensor_of_block(a.blk0, a.nt, b);
  const posu_adam_dev_tensor& t = a.t[ti];
  // bias corrections from the device step, in double as the host does for posu_adam_step
  const double step = static_cast<double>(*t.step);
  const double bc1 = 1.0 - pow(a.beta1, step);
  const double bc2 = 1.0 - pow(a.beta2, step);
  AdamCoef c;
  c.step_size = static_cast<float>(a.lr / bc1);
  c.inv_bc2s = static_cast<float>(1.0 / sqrt(bc2));
  c.beta1 = static_cast<float>(a.beta1);
  c.beta2 = static_cast<float>(a.beta2);
  c.omb1 = static_cast<float>(1.0 - a.beta1);
  c.omb2 = static_cast<float>(1.0 - a.beta2);
  c.eps = a.eps;
  c.wd = a.wd;
  // gradient multiplier = 1 / scale * clip, clip = min(1, max_norm / (||g|| / scale + 1e-6))
  // (torch.nn.utils.clip_grad_norm_, in f32)
  const float inv = a.scale ? static_cast<float>(1.0 / static_cast<double>(*a.scale)) : 1.f;
  float gmul = inv;
  if (a.sumsq && a.max_norm > 0.f) {
    const float norm = static_cast<float>(sqrt(*a.sumsq)) * inv;
    gmul = inv * fminf(1.f, a.max_norm / (norm + 1e-6f));
  }
  const long long e0 = (b - a.blk0[ti]) * kAdamChunk;
  adam_chunk<true>(t, e0, min(t.n, e0 + kAdamChunk), c, gmul);
}

// Gradient statistics (posu_grad_stats): same launch table and chunking as Adam.
struct GradLaunch {
  posu_grad_tensor t[kAdamTensors];
  long long blk0[kAdamTensors + 1];
  long long part0;   // this launch's first slot in `partials`
  int nt, unscale;
  const float* scale;
  float* found_inf;
  double* partials;   // null: no sum of squares
};

__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// fixed-order block sum of one double per thread (N threads, a multiple of 64); thread 0 has it
template <int N>
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double wsum[N / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < N / 64; ++w) s += wsum[w];
  return s;
}

__global__ __launch_bounds__(kAdamThreads) void grad_stats_kernel(const GradLaunch a) {
  const long long b = blockIdx.x;
  const int ti = tensor_of_block(a.blk0, a.nt, b);
  const posu_grad_tensor& t = a.t[ti];
  const long long e0 = (b - a.blk0[ti]) * kAdamChunk;
  const long long e1 = min(t.n, e0 + kAdamChunk);
  const float inv = a.unscale ? static_cast<float>(1.0 / static_cast<double>(*a.scale)) : 1.f;
  bool bad = false;
  double ss = 0.0;
  if ((reinterpret_cast<size_t>(t.g) & 15) == 0 && e1 - e0 == kAdamChunk) {
    float4 g4[kAdamVec];
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u)
      g4[u] = reinterpret_cast<const float4*>(t.g)[e0 / 4 + u * kAdamThreads + threadIdx.x];
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u) {
      float g[4] = {g4[u].x, g4[u].y, g4[u].z, g4[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        bad |= non_finite(g[k]);
        if (a.unscale) g[k] *= inv;
        ss += static_cast<double>(g[k]) * static_cast<double>(g[k]);
      }
      if (a.unscale)
        reinterpret_cast<float4*>(t.g)[e0 / 4 + u * kAdamThreads + threadIdx.x] = make_float4(g[0], g[1], g[2], g[3]);
    }
  } else {
    for (long long i = e0 + threadIdx.x; i < e1; i += kAdamThreads) {   // ragged / unaligned tail
      float g = t.g[i];
      bad |= non_finite(g);
      if (a.unscale) t.g[i] = g = g * inv;
      ss += static_cast<double>(g) * static_cast<double>(g);
    }
  }
  if (bad) *a.found_inf = 1.f;   // every writer stores the same value: no ordering needed
  if (a.partials) {
    const double s = block_sum_f64<kAdamThreads>(ss);
    if (threadIdx.x == 0) a.partials[a.part0 + b] = s;
  }
}

// second stage: the per-block partials in a fixed order (thread i takes i, i + 256, ...; then the
// block sum), so the result is the same bits on every run
__global__ __launch_bounds__(kAdamThreads) void grad_sumsq_kernel(const double* partials, long long n, double* out) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += kAdamThreads) s += partials[i];
  s = block_sum_f64<kAdamThreads>(s);
  if (threadIdx.x == 0) *out = s;
}

// torch's _amp_update_scale_ on device scalars
__global__ void loss_scale_update_kernel(float* scale, int* tracker, const float* found_inf, float growth,
                                         float backoff, int interval) {
  if (*found_inf != 0.f) {
    *scale *= backoff;
    *tracker = 0;
    return;
  }
  const int good = *tracker + 1;
  if (good < interval) {
    *tracker = good;
    return;
  }
  const float grown = *scale * growth;
  if (!non_finite(grown)) *scale = grown;   // the scale never grows to inf
  *tracker = 0;
}

long long chunks_of(long long n) { return (n + kAdamChunk - 1) / kAdamChunk; }

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" int posu_adam_step(const posu_adam_tensor* tensors, int ntensors, double lr, double beta1, double beta2,
                              double eps, double weight_decay, long long step, void* stream) {
  POSU_REQUIRE(ntensors >= 0 && (ntensors == 0 || tensors), "posu_adam_step: null tensor table");
  POSU_REQUIRE(step >= 1, "posu_adam_step: step counts from 1");
  POSU_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
               "posu_adam_step: bad hyper-parameters");
  for (int i = 0; i < ntensors; ++i)
    POSU_REQUIRE(tensors[i].n >= 0 && (tensors[i].n == 0 || (tensors[i].p && tensors[i].g && tensors[i].m &&
                                                               tensors[i].v)),
                 "posu_adam_step: tensor " + std::to_string(i) + " has a null pointer");
  const double bc1 = 1.0 - std::pow(beta1, static_cast<double>(step));
  const double bc2 = 1.0 - std::pow(beta2, static_cast<double>(step));
  AdamLaunch a{};
  a.step_size = static_cast<float>(lr / bc1);
  a.inv_bc2s = static_cast<float>(1.0 / std::sqrt(bc2));
  a.beta1 = static_cast<float>(beta1);
  a.beta2 = static_cast<float>(beta2);
  a.omb1 = static_cast<float>(1.0 - beta1);
  a.omb2 = static_cast<float>(1.0 - beta2);
  a.eps = static_cast<float>(eps);
  a.wd = static_cast<float>(weight_decay);
  hipStream_t s = as_stream(stream);
  int i = 0;
  while (i < ntensors) {
    a.nt = 0;
    long long blocks = 0;
    for (; i < ntensors && a.nt < kAdamTensors; ++i) {
      if (tensors[i].n == 0) continue;
      a.t[a.nt] = tensors[i];
      a.blk0[a.nt] = blocks;
      blocks += (tensors[i].n + kAdamChunk - 1) / kAdamChunk;
      ++a.nt;
    }
    a.blk0[a.nt] = blocks;
    if (a.nt == 0) break;
    POSU_REQUIRE(blocks < (1LL << 31), "posu_adam_step: too many blocks in one launch");
    hipLaunchKernelGGL(adam_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kAdamThreads), 0, s, a);
    if (int st = check_launch("posu_adam_step")) return st;
  }
  return POSU_OK;
}

extern "C" long long posu_grad_stats_workspace(const posu_grad_tensor* tensors, int ntensors) {
  if (ntensors < 0 || (ntensors > 0 && !tensors)) return -1;
  long long blocks = 0;
  for (int i = 0; i < ntensors; ++i) {
    if (tensors[i].n < 0) return -1;
    blocks += chunks_of(tensors[i].n);
  }
  return static_cast<long long>(sizeof(double)) * std::max(blocks, 1LL);
}

extern "C" int posu_grad_stats(const posu_grad_tensor* tensors, int ntensors, const float* scale, int unscale,
                               float* found_inf, double* sumsq, void* workspace, long long workspace_bytes,
                               void* stream) {
  POSU_REQUIRE(ntensors >= 0 && (ntensors == 0 || tensors), "posu_grad_stats: null tensor table");
  POSU_REQUIRE(found_inf, "posu_grad_stats: null found_inf");
  POSU_REQUIRE(!unscale || scale, "posu_grad_stats: unscale needs the scale");
  for (int i = 0; i < ntensors; ++i) {
    POSU_REQUIRE(tensors[i].n >= 0, "posu_grad_stats: tensor " + std::to_string(i) + " has a negative size");
    POSU_REQUIRE(tensors[i].n == 0 || tensors[i].g,
                 "posu_grad_stats: tensor " + std::to_string(i) + " has a null pointer");
  }
  if (sumsq)
    POSU_REQUIRE(workspace && workspace_bytes >= posu_grad_stats_workspace(tensors, ntensors),
                 "posu_grad_stats: workspace too small (posu_grad_stats_workspace)");
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(found_inf, 0, sizeof(float), s) != hipSuccess) return check_launch("posu_grad_stats");
  GradLaunch a{};
  a.scale = scale;
  a.unscale = unscale != 0;
  a.found_inf = found_inf;
  a.partials = sumsq ? static_cast<double*>(workspace) : nullptr;
  for (int i = 0; i < ntensors;) {
    a.nt = 0;
    long long blocks = 0;
    for (; i < ntensors && a.nt < kAdamTensors; ++i, ++a.nt) {   // (an empty tensor takes no block)
      a.t[a.nt] = tensors[i];
      a.blk0[a.nt] = blocks;
      blocks += chunks_of(tensors[i].n);
    }
    a.blk0[a.nt] = blocks;
    if (blocks == 0) continue;
    POSU_REQUIRE(blocks < (1LL << 31), "posu_grad_stats: too many blocks in one launch");
    hipLaunchKernelGGL(grad_stats_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kAdamThreads), 0, s, a);
    if (int st = check_launch("posu_grad_stats")) return st;
    a.part0 += blocks;
  }
  if (sumsq) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(1), dim3(kAdamThreads), 0, s, a.partials, a.part0, sumsq);
    if (int st = check_launch("posu_grad_stats")) return st;
  }
  return POSU_OK;
}

extern "C" int posu_adam_step_dev(const posu_adam_dev_tensor* tensors, int ntensors, double lr, double beta1,
                                  double beta2, double eps, double weight_decay, const float* found_inf,
                                  const float* scale, const double* sumsq, double max_norm, void* stream) {
  POSU_REQUIRE(ntensors >= 0 && (ntensors == 0 || tensors), "posu_adam_step_dev: null tensor table");
  POSU_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
               "posu_adam_step_dev: bad hyper-parameters");
  POSU_REQUIRE(!(max_norm > 0.0) || sumsq, "posu_adam_step_dev: max_norm needs the gradients' sum of squares");
  for (int i = 0; i < ntensors; ++i) {
    POSU_REQUIRE(tensors[i].n >= 0, "posu_adam_step_dev: tensor " + std::to_string(i) + " has a negative size");
    POSU_REQUIRE(tensors[i].step && (tensors[i].n == 0 || (tensors[i].p && tensors[i].g && tensors[i].m &&
                                                             tensors[i].v)),
                 "posu_adam_step_dev: tensor " + std::to_string(i) + " has a null pointer");
  }
  AdamDevLaunch a{};
  a.lr = lr;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = static_cast<float>(eps);
  a.wd = static_cast<float>(weight_decay);
  a.max_norm = max_norm > 0.0 ? static_cast<float>(max_norm) : 0.f;
  a.found_inf = found_inf;
  a.scale = scale;
  a.sumsq = sumsq;
  hipStream_t s = as_stream(stream);
  for (int i = 0; i < ntensors;) {
    // an empty tensor keeps its record (its step still counts) and takes no block
    a.nt = 0;
    long long blocks = 0;
    for (; i < ntensors && a.nt < kAdamTensors; ++i, ++a.nt) {
      a.t[a.nt] = tensors[i];
      a.blk0[a.nt] = blocks;
      blocks += chunks_of(tensors[i].n);
    }
    a.blk0[a.nt] = blocks;
    POSU_REQUIRE(blocks < (1LL << 31), "posu_adam_step_dev: too many blocks in one launch");
    hipLaunchKernelGGL(adam_dev_prologue, dim3(1), dim3(kAdamTensors), 0, s, a);
    if (int st = check_launch("posu_adam_step_dev")) return st;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(adam_dev_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kAdamThreads), 0, s, a);
    if (int st = check_launch("posu_adam_step_dev")) return st;
  }
  return POSU_OK;
}

extern "C" int posu_loss_scale_update(float* scale, int* growth_tracker, const float* found_inf, double growth,
                                      double backoff, int growth_interval, void* stream) {
  POSU_REQUIRE(scale && growth_tracker, "posu_loss_scale_update: null scale / growth_tracker");
  POSU_REQUIRE(found_inf, "posu_loss_scale_update: null found_inf");
  POSU_REQUIRE(growth >= 1.0 && backoff > 0.0 && backoff <= 1.0,
               "posu_loss_scale_update: growth >= 1 and 0 < backoff <= 1");
  POSU_REQUIRE(growth_interval >= 1, "posu_loss_scale_update: growth_interval < 1");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, as_stream(stream), scale, growth_tracker,
                     found_inf, static_cast<float>(growth), static_cast<float>(backoff), growth_interval);
  return check_launch("posu_loss_scale_update");
}
