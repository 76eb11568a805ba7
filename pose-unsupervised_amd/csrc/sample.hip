// A training batch's samples, JointsDatasetCompatible.__getitem__ (lib/dataset/joints_dataset_compatible.py
// :111-201) for N records per enqueue:
//   sample images          : the flip (:156), cv2.warpAffine (:162-165, warp_common.h), torchvision's
//                            ColorJitter on the PIL image (:67-71, :168-172) and ToTensor + Normalize (:173),
//                            one thread per output pixel with the three channels in registers;
//   sample joints/targets  : fliplr_joints (lib/utils/transforms.py:50-64), the joints' affine (:175-177)
//                            and generate_heatmap (:207-253), one block per (record, joint).
#include "posu_common.h"
#include "warp_common.h"

namespace posu {
namespace {

// torchvision ColorJitter's fn_ids
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

// Everything below restates C code that rounds every operation on its own: no FMA contraction.
#pragma clang fp contract(off)

// PIL Image.convert('L') of RGB (Convert.c)
__device__ __forceinline__ int pil_l(const int* c) {
  return (19595 * c[0] + 38470 * c[1] + 7471 * c[2] + 0x8000) >> 16;
}

// PIL Image.blend(degenerate, image, f) per byte (Blend.c): d + f * (x - d) in f32, truncated for
// 0 <= f <= 1, otherwise clipped to [0, 255] and truncated
__device__ __forceinline__ int pil_blend(int d, int x, float f) {
  const float t = static_cast<float>(d) + f * static_cast<float>(x - d);
  if (f >= 0.f && f <= 1.f) return static_cast<int>(t);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : static_cast<int>(t));
}

// PIL RGB -> HSV (Convert.c rgb2hsv_row): f32 quotients; the sum with the constant and the fmod in
// double, each rounded to f32; grey pixels give H = S = 0
__device__ __forceinline__ void pil_rgb2hsv(const int* c, int* hsv) {
  const int r = c[0], g = c[1], b = c[2];
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  hsv[2] = maxc;
  if (minc == maxc) {
    hsv[0] = hsv[1] = 0;
    return;
  }
  const float cr = static_cast<float>(maxc - minc);
  const float s = cr / static_cast<float>(maxc);
  const float rc = static_cast<float>(maxc - r) / cr;
  const float gc = static_cast<float>(maxc - g) / cr;
  const float bc = static_cast<float>(maxc - b) / cr;
  float h;
  if (r == maxc) {
    h = bc - gc;
  } else if (g == maxc) {
    h = static_cast<float>(2.0 + static_cast<double>(rc) - static_cast<double>(bc));
  } else {
    h = static_cast<float>(4.0 + static_cast<double>(gc) - static_cast<double>(rc));
  }
  const double t = static_cast<double>(h) / 6.0 + 1.0;   // in [5/6, 11/6]: fmod(t, 1.0) = t - trunc(t), exact
  h = static_cast<float>(t - trunc(t));
  hsv[0] = static_cast<int>(static_cast<double>(h) * 255.0);
  hsv[1] = static_cast<int>(static_cast<double>(s) * 255.0);
}

// PIL HSV -> RGB (Convert.c hsv2rgb): sector and remainder from h * 6.0 / 255.0 in double (the remainder
// rounded to f32), fs = s / 255.0 rounded to f32, fs * f in f32, the products in double, C round()
__device__ __forceinline__ void pil_hsv2rgb(const int* hsv, int* c) {
  const int v = hsv[2];
  if (hsv[1] == 0) {
    c[0] = c[1] = c[2] = v;
    return;
  }
  const double h6 = static_cast<double>(hsv[0]) * 6.0 / 255.0;
  const double fl = floor(h6);
  const float f = static_cast<float>(h6 - fl);
  const float fs = static_cast<float>(static_cast<double>(hsv[1]) / 255.0);
  const double vd = static_cast<double>(v);
  const float fsf = fs * f;
  const int p = min(max(static_cast<int>(round(vd * (1.0 - static_cast<double>(fs)))), 0), 255);
  const int q = min(max(static_cast<int>(round(vd * (1.0 - static_cast<double>(fsf)))), 0), 255);
  const int t = min(
      max(static_cast<int>(round(vd * (1.0 - static_cast<double>(fs) * (1.0 - static_cast<double>(f))))), 0), 255);
  switch (static_cast<int>(fl) % 6) {
    case 0: c[0] = v, c[1] = t, c[2] = p; break;
    case 1: c[0] = q, c[1] = v, c[2] = p; break;
    case 2: c[0] = p, c[1] = v, c[2] = t; break;
    case 3: c[0] = p, c[1] = q, c[2] = v; break;
    case 4: c[0] = t, c[1] = p, c[2] = v; break;
    default: c[0] = v, c[1] = p, c[2] = q; break;
  }
}

// numpy's float32 exp as its AVX2 / AVX512F kernels compute it (numpy/core/src/umath/loops_exponent_log:
// simd_exp_FLOAT), which is what generate_heatmap's np.exp gives on the hosts the reference trains on.  It is
// faithful, not correctly rounded, so expf does not reproduce it: x log2(e) rounded with the 1.5 * 2^23 add,
// Cody-Waite reduction in two fused steps, a (5, 2) rational approximation in Horner form with fused
// multiply-adds, one division, the exponent added.  For the Gaussian's arguments, [-9, 0]: no range clamps.
__device__ __forceinline__ float numpy_expf(float x) {
  float q = x * 1.44269504088896341f;
  q = (q + 12582912.f) - 12582912.f;
  float r = fmaf(q, -6.93145752e-1f, x);
  r = fmaf(q, -1.42860677e-6f, r);
  float num = fmaf(5.082762527590693718096e-04f, r, 6.757896990527504603057e-03f);
  num = fmaf(num, r, 5.114512081637298353406e-02f);
  num = fmaf(num, r, 2.473615434895520810817e-01f);
  num = fmaf(num, r, 7.257664613233124478488e-01f);
  num = fmaf(num, r, 9.999999999980870924916e-01f);
  float den = fmaf(2.159509375685829852307e-02f, r, -2.742335390411667452936e-01f);
  den = fmaf(den, r, 1.f);
  return ldexpf(num / den, static_cast<int>(q));
}

// sum over the block's 256 threads (4 waves), valid in thread 0
__device__ __forceinline__ unsigned block_sum_u32(unsigned v, unsigned* lds) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// Grid (ceil(dh * dw / 256), N): a block stays inside one record, so the record's jitter order is uniform
// over it.  PASS 0 is the contrast pre-pass: the warp and the point operations that precede the contrast
// step, then the exact integer sum of L into ws[n] (one 64-bit atomic per block).  PASS 1 is the sample:
// it reads the sum where the contrast step stands.
template <int PASS>
__global__ __launch_bounds__(256) void sample_images_kernel(
    const unsigned char* __restrict__ src, const long long* __restrict__ src_off, const int* __restrict__ src_hw,
    const double* __restrict__ Mall, const unsigned char* __restrict__ flip, const posu_jitter* __restrict__ jitter,
    int bgr, int dh, int dw, int mode, const float* __restrict__ mean, const float* __restrict__ stdv,
    unsigned long long* __restrict__ ws, void* __restrict__ out) {
  __shared__ unsigned lds[4];
  const int n = blockIdx.y;
  const bool active = jitter != nullptr && jitter[n].active != 0;
  if (PASS == 0 && !active) return;
  const int npix = dh * dw;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool live = p < npix;
  const int y = live ? p / dw : 0, x = live ? p - y * dw : 0;
  int c[3] = {0, 0, 0};   // the source's channel order until the jitter, RGB inside it
  if (live) {
    const int H = src_hw[2 * n], W = src_hw[2 * n + 1];
    const WarpTaps t = warp_taps(Mall + 6 * n, x, y, H, W);
    const unsigned char* S = src + src_off[n];
    const bool fl = flip != nullptr && flip[n] != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = warp_channel(S, H, W, 3, k, t, fl);
  }
  if (active) {
    const posu_jitter jr = jitter[n];
    if (bgr) {
      const int t = c[0];
      c[0] = c[2];
      c[2] = t;
    }
    for (int k = 0; k < 4; ++k) {
      const int op = jr.order[k];
      if (op == OP_BRIGHTNESS) {
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = pil_blend(0, c[i], jr.brightness);
      } else if (op == OP_CONTRAST) {
        if (PASS == 0) {
          const unsigned s = block_sum_u32(live ? static_cast<unsigned>(pil_l(c)) : 0u, lds);
          if (threadIdx.x == 0) atomicAdd(ws + n, static_cast<unsigned long long>(s));
          return;
        }
        // ImageEnhance.Contrast: int(ImageStat.Stat(L).mean[0] + 0.5)
        const int grey = static_cast<int>(static_cast<double>(ws[n]) / static_cast<double>(npix) + 0.5);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = pil_blend(grey, c[i], jr.contrast);
      } else if (op == OP_SATURATION) {
        const int l = pil_l(c);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = pil_blend(l, c[i], jr.saturation);
      } else if (op == OP_HUE) {
        int hsv[3];
        pil_rgb2hsv(c, hsv);
        hsv[0] = (hsv[0] + jr.hue_shift) & 255;
        pil_hsv2rgb(hsv, c);
      }
    }
    if (bgr) {
      const int t = c[0];
      c[0] = c[2];
      c[2] = t;
    }
  }
  if (PASS == 0 || !live) return;
  if (mode == 0) {
    unsigned char* o = static_cast<unsigned char*>(out) + (static_cast<long long>(n) * npix + p) * 3;
    o[0] = static_cast<unsigned char>(c[0]);
    o[1] = static_cast<unsigned char>(c[1]);
    o[2] = static_cast<unsigned char>(c[2]);
  } else {
    float* o = static_cast<float*>(out) + static_cast<long long>(n) * 3 * npix + p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float t = static_cast<float>(c[k]) / 255.f;
      o[static_cast<long long>(k) * npix] = (t - mean[k]) / stdv[k];
    }
  }
}

// One block per (record n, joint j).  Every thread derives the joint (a few f64 operations, uniform over
// the block), thread 0 stores it, all threads paint the map.
//   flip:   x = W - x - 1, the pair swap of joints and vis (joint j reads perm[j]), joints * vis;
//   affine: [x, y, 1] . trans^T for joints with vis[:, 0] > 0.  numpy hands this product to BLAS, whose
//           kernels fuse one multiply-add: with two or more visible joints (gemm) fma(y, t1, x * t0) + t2,
//           with exactly one (gemv, the .squeeze() case) fma(x, t0, y * t1) + t2.  Both are reproduced;
//   target: gaussian_targets_kernel's (datapath.hip) with mu = int(joint / stride + 0.5) in f64 and the
//           Gaussian through numpy's own float32 exp (numpy_expf above).
__global__ __launch_bounds__(256) void sample_joints_targets_kernel(
    const double* __restrict__ joints, const double* __restrict__ vis, const unsigned char* __restrict__ flip,
    const int* __restrict__ src_hw, const int* __restrict__ perm, const double* __restrict__ Mall,
    const unsigned char* __restrict__ zero_w, int J, double stride_x, double stride_y, int hw, int hh, double sigma,
    double* __restrict__ joints_out, double* __restrict__ vis_out, float* __restrict__ target,
    float* __restrict__ weight) {
  const long long nj = blockIdx.x;
  const int n = static_cast<int>(nj / J), j = static_cast<int>(nj - static_cast<long long>(n) * J);
  const bool fl = flip != nullptr && flip[n] != 0;
  const long long from = static_cast<long long>(n) * J + (fl ? perm[j] : j);
  double x = joints[2 * from], y = joints[2 * from + 1];
  const double v0 = vis[2 * from], v1 = vis[2 * from + 1];
  if (fl) {
    x = static_cast<double>(src_hw[2 * n + 1]) - x - 1.0;
    x = x * v0;
    y = y * v1;
  }
  if (v0 > 0.0) {
    int nvis = 0;
    for (int k = 0; k < J; ++k) nvis += vis[2 * (static_cast<long long>(n) * J + k)] > 0.0;
    const double* t = Mall + 6 * n;
    double ox, oy;
    if (nvis >= 2) {
      ox = fma(y, t[1], x * t[0]) + t[2];
      oy = fma(y, t[4], x * t[3]) + t[5];
    } else {
      ox = fma(x, t[0], y * t[1]) + t[2];
      oy = fma(x, t[3], y * t[4]) + t[5];
    }
    x = ox;
    y = oy;
  }
  const double tmp = sigma * 3.0;
  // Python int(): truncation toward zero
  const int mu_x = static_cast<int>(trunc(x / stride_x + 0.5));
  const int mu_y = static_cast<int>(trunc(y / stride_y + 0.5));
  const int ul_x = static_cast<int>(trunc(mu_x - tmp)), ul_y = static_cast<int>(trunc(mu_y - tmp));
  const int br_x = static_cast<int>(trunc(mu_x + tmp + 1.0)), br_y = static_cast<int>(trunc(mu_y + tmp + 1.0));
  const bool outside = ul_x >= hw || ul_y >= hh || br_x < 0 || br_y < 0;
  const float v = outside ? 0.f : static_cast<float>(v0);
  if (threadIdx.x == 0) {
    joints_out[2 * nj] = x;
    joints_out[2 * nj + 1] = y;
    vis_out[2 * nj] = v0;
    vis_out[2 * nj + 1] = v1;
    weight[nj] = (zero_w && zero_w[n]) ? 0.f : v;
  }
  const double size = 2.0 * tmp + 1.0;
  const float c0 = static_cast<float>(floor(size / 2.0));   // x0 = y0 = size // 2
  const float den = static_cast<float>(2.0 * sigma * sigma);
  float* tg = target + nj * hh * hw;
  for (int i = threadIdx.x; i < hh * hw; i += 256) {
    const int py = i / hw, px = i - py * hw;
    float g = 0.f;
    if (v > 0.5f && px >= ul_x && px < br_x && py >= ul_y && py < br_y) {
      const float dx = static_cast<float>(px - ul_x) - c0, dy = static_cast<float>(py - ul_y) - c0;
      g = numpy_expf(-(dx * dx + dy * dy) / den);
    }
    tg[i] = g;
  }
}
#pragma clang fp contract(on)

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" long long posu_sample_workspace(int N) {
  return N < 0 ? -1 : static_cast<long long>(N) * static_cast<long long>(sizeof(unsigned long long));
}

extern "C" int posu_sample_images(const unsigned char* src, const long long* src_off, const int* src_hw, int C,
                                  const double* M, const unsigned char* flip, const posu_jitter* jitter,
                                  int contrast, int bgr, int N, int dh, int dw, int mode, const float* mean,
                                  const float* std, void* workspace, long long workspace_bytes, void* out,
                                  void* stream) {
  POSU_REQUIRE(src && src_off && src_hw && M && out, "posu_sample_images: null pointer");
  POSU_REQUIRE(C == 3, "posu_sample_images: bad shape (C must be 3)");
  POSU_REQUIRE(N >= 0 && N <= 65535 && dh > 0 && dw > 0 && static_cast<long long>(dh) * dw <= (1LL << 30),
               "posu_sample_images: bad shape");
  POSU_REQUIRE(mode == 0 || mode == 1, "posu_sample_images: mode must be 0 (uint8 HWC) or 1 (normalised f32 NCHW)");
  POSU_REQUIRE(mode == 0 || (mean && std), "posu_sample_images: mode 1 needs mean and std");
  POSU_REQUIRE(!contrast || jitter, "posu_sample_images: null pointer (contrast without jitter records)");
  POSU_REQUIRE(!jitter || (workspace && workspace_bytes >= posu_sample_workspace(N)),
               "posu_sample_images: workspace too small (posu_sample_workspace)");
  if (N == 0) return POSU_OK;
  const dim3 grid((dh * dw + 255) / 256, N);
  unsigned long long* ws = static_cast<unsigned long long*>(workspace);
  if (contrast) {
    if (hipMemsetAsync(ws, 0, static_cast<size_t>(posu_sample_workspace(N)), as_stream(stream)) != hipSuccess)
      return check_launch("posu_sample_images (workspace)");
    hipLaunchKernelGGL(sample_images_kernel<0>, grid, dim3(256), 0, as_stream(stream), src, src_off, src_hw, M, flip,
                       jitter, bgr, dh, dw, mode, mean, std, ws, out);
  }
  hipLaunchKernelGGL(sample_images_kernel<1>, grid, dim3(256), 0, as_stream(stream), src, src_off, src_hw, M, flip,
                     jitter, bgr, dh, dw, mode, mean, std, ws, out);
  return check_launch("posu_sample_images");
}

extern "C" int posu_sample_joints_targets(const double* joints, const double* vis, const unsigned char* flip,
                                          const int* src_hw, const int* perm, const double* M,
                                          const unsigned char* zero_weight, int N, int J, int image_w, int image_h,
                                          int hm_w, int hm_h, double sigma, double* joints_out, double* vis_out,
                                          float* target, float* weight, void* stream) {
  POSU_REQUIRE(joints && vis && M && joints_out && vis_out && target && weight,
               "posu_sample_joints_targets: null pointer");
  POSU_REQUIRE(!flip || (src_hw && perm), "posu_sample_joints_targets: null pointer (flip needs src_hw and perm)");
  POSU_REQUIRE(N >= 0 && J > 0 && image_w > 0 && image_h > 0 && hm_w > 0 && hm_h > 0 && sigma > 0 &&
                   static_cast<long long>(hm_w) * hm_h <= (1LL << 30),
               "posu_sample_joints_targets: bad shape");
  POSU_REQUIRE(static_cast<long long>(N) * J <= 0x7fffffffLL, "posu_sample_joints_targets: shape too large");
  if (N == 0) return POSU_OK;
  hipLaunchKernelGGL(sample_joints_targets_kernel, dim3(N * J), dim3(256), 0, as_stream(stream), joints, vis, flip,
                     src_hw, perm, M, zero_weight, J, static_cast<double>(image_w) / hm_w,
                     static_cast<double>(image_h) / hm_h, hm_w, hm_h, sigma, joints_out, vis_out, target, weight);
  return check_launch("posu_sample_joints_targets");
}
