// Fundamental matrices from 2-D correspondences on the device: a batched least-median-of-squares
// estimator over the normalised 8-point algorithm, the producer of the {(subject, i, j): 3x3} table
// FundamentalLoss reads (the reference makes it with cv2.findFundamentalMat(..., cv2.FM_LMEDS) in
// run/test/generate_fundamental_matirx.py:36-103).  fp64 throughout; include/posu.h has the definition.
//
// Three launches per call, no host read between them:
//   k_hypotheses  one lane per (problem, hypothesis): 8 distinct valid rows from the Philox stream,
//                 sorted, Hartley normalisation, the 8 x 9 system, its null vector by jacobi_columns,
//                 rank 2, denormalisation.  The matrices live in registers (one wave per SIMD).
//   k_score       one block per (problem, hypothesis): the exact element of rank n / 2 of the rows'
//                 symmetric epipolar errors by a radix select over their bit patterns (non-negative
//                 doubles order like integers).  8 passes of 8 bits, each recomputing the errors into
//                 a 256-bin LDS histogram: nothing is stored per row, so N has no cap.
//   k_finalize    one block per problem: the smallest median (ties to the lowest h), sigma, the inlier
//                 mask, and the refit over all inliers: two reductions for the normalisation, the 45
//                 sums of the 9 x 9 Gram matrix, jacobi_columns on it, rank 2, denormalisation, scale.
// Sums over rows are taken in a fixed order (lane stride, wave butterfly, waves in order): the same
// inputs give the same bits.  Nothing here is tuned; k_score does P H N errors per pass and is the cost.
#include <cmath>

#include "geometry_common.h"
#include "philox_common.h"

namespace posu {
namespace {

constexpr int kSample = 8;            // rows of a hypothesis
constexpr int kMaxRejects = 64;       // rejected candidates before a hypothesis is given up
constexpr int kHypLanes = 64;
constexpr int kThreads = 256;         // k_score, k_finalize, k_residual_stats
constexpr int kWaves = kThreads / 64;
constexpr int kMaxProblems = 65535;   // grid y
constexpr int kMaxHypotheses = 1 << 20;
constexpr int kMaxRows = 1 << 26;
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;
constexpr double kSigmaFloor = 1e-3;  // px

// x -> s (x - c): centroid to the origin, mean distance sqrt(2)
struct Hartley {
  double cx, cy, s;
};

// the row of the system for one correspondence: a . vec(F) = x_j^T F x_i
__device__ __forceinline__ void system_row(double xi, double yi, double xj, double yj, double (&a)[9]) {
  a[0] = xj * xi, a[1] = xj * yi, a[2] = xj;
  a[3] = yj * xi, a[4] = yj * yi, a[5] = yj;
  a[6] = xi, a[7] = yi, a[8] = 1.0;
}

// V's column under A's column of the smallest norm (the first of equals): jacobi_columns leaves
// A = U diag(s), so this is the right singular vector of the smallest singular value
template <int ROWS>
__device__ __forceinline__ void null_vector(double (&A)[ROWS][9], double (&f)[9]) {
  double V[9][9];
  jacobi_columns<ROWS, 9>(A, V);
  double best = 0;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    double n = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) n += A[r][c] * A[r][c];
    if (c == 0 || n < best) {
      best = n;
#pragma unroll
      for (int k = 0; k < 9; ++k) f[k] = V[k][c];
    }
  }
}

// f, the solution in normalised coordinates -> F: the smallest singular value set to zero (3 x 3
// Jacobi: F^ = sum over the two kept columns c of (U s)_c V_c^T), then T_j^T F^ T_i
__device__ __forceinline__ void finish_matrix(const double (&f)[9], const Hartley& hi, const Hartley& hj,
                                              double (&F)[9]) {
  double A[3][3], V[3][3], n[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) A[r][c] = f[3 * r + c];
  jacobi_columns<3, 3>(A, V);
#pragma unroll
  for (int c = 0; c < 3; ++c) n[c] = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c];
  int drop = 0;
  if (n[1] < n[drop]) drop = 1;
  if (n[2] < (drop ? n[1] : n[0])) drop = 2;
  double R[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double s = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) s += c == drop ? 0.0 : A[r][c] * V[k][c];
      R[r][k] = s;
    }
  double M[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    M[r][0] = R[r][0] * hi.s;
    M[r][1] = R[r][1] * hi.s;
    M[r][2] = R[r][2] - hi.s * (hi.cx * R[r][0] + hi.cy * R[r][1]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    F[c] = hj.s * M[0][c];
    F[3 + c] = hj.s * M[1][c];
    F[6 + c] = M[2][c] - hj.s * (hj.cx * M[0][c] + hj.cy * M[1][c]);
  }
}

// max(d_i^2, d_j^2), the squared distances of x_i and x_j to the epipolar lines F^T x_j and F x_i
__device__ __forceinline__ double epipolar_error(const double (&F)[9], double xi, double yi, double xj, double yj) {
  const double a = F[0] * xi + F[1] * yi + F[2], b = F[3] * xi + F[4] * yi + F[5], c = F[6] * xi + F[7] * yi + F[8];
  const double s = xj * a + yj * b + c, s2 = s * s;
  const double at = F[0] * xj + F[3] * yj + F[6], bt = F[1] * xj + F[4] * yj + F[7];
  return fmax(s2 / (at * at + bt * bt), s2 / (a * a + b * b));   // fmax passes a NaN only when both are
}

// the error as the integer it is ordered by; a NaN counts as +inf
__device__ __forceinline__ unsigned long long error_bits(const double (&F)[9], const double* row) {
  const double e = epipolar_error(F, row[0], row[1], row[2], row[3]);
  return e == e ? static_cast<unsigned long long>(__double_as_longlong(e)) : kInfBits;
}

// K sums over the block, every thread gets them: wave butterflies, then the waves in order
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double* red) {
  __syncthreads();   // red may still be read from the previous use
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double w = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) red[k * kWaves + (threadIdx.x >> 6)] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += red[k * kWaves + w];
    v[k] = s;
  }
}

// ------------------------------------------------------------------ hypotheses
__global__ __launch_bounds__(kHypLanes) void k_hypotheses(const double* __restrict__ pts,
                                                          const unsigned char* __restrict__ valid, int N, int H,
                                                          uint32_t seed_lo, uint32_t seed_hi,
                                                          double* __restrict__ Fh, int* __restrict__ samples) {
  const int h = blockIdx.x * kHypLanes + threadIdx.x, p = blockIdx.y;
  if (h >= H) return;
  const double* q = pts + static_cast<size_t>(p) * N * 4;
  const unsigned char* ok = valid ? valid + static_cast<size_t>(p) * N : nullptr;
  const size_t slot = static_cast<size_t>(p) * H + h;

  // every word either takes a row or is a rejection: at most 8 + 64 words
  int rows[kSample], taken = 0, rejected = 0;
#pragma unroll
  for (int k = 0; k < kSample; ++k) rows[k] = -1;
  for (uint32_t b = 0; taken < kSample && rejected < kMaxRejects; ++b) {
    const Philox w = philox4x32_10(b, static_cast<uint32_t>(h), static_cast<uint32_t>(p), 0u, seed_lo, seed_hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (taken < kSample && rejected < kMaxRejects) {
        const int cand = bounded(w.c[i], N);
        bool bad = ok && !ok[cand];
#pragma unroll
        for (int k = 0; k < kSample; ++k) bad |= rows[k] == cand;
        if (bad) {
          ++rejected;
        } else {
#pragma unroll
          for (int k = 0; k < kSample; ++k)
            if (k == taken) rows[k] = cand;
          ++taken;
        }
      }
    }
  }
  if (taken < kSample) {
#pragma unroll
    for (int k = 0; k < kSample; ++k) samples[slot * kSample + k] = -1;
#pragma unroll
    for (int k = 0; k < 9; ++k) Fh[slot * 9 + k] = __longlong_as_double(0x7FF8000000000000ll);
    return;
  }
  // ascending: hypotheses that drew the same rows in another order are the same hypothesis, bit for bit
#pragma unroll
  for (int pass = 0; pass < kSample; ++pass)
#pragma unroll
    for (int k = pass & 1; k + 1 < kSample; k += 2) {
      const int lo = min(rows[k], rows[k + 1]), hi = max(rows[k], rows[k + 1]);
      rows[k] = lo, rows[k + 1] = hi;
    }
#pragma unroll
  for (int k = 0; k < kSample; ++k) samples[slot * kSample + k] = rows[k];

  double x[kSample][4], sum[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kSample; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      x[k][c] = q[static_cast<size_t>(rows[k]) * 4 + c];
      sum[c] += x[k][c];
    }
  Hartley hi = {sum[0] / kSample, sum[1] / kSample, 0.0}, hj = {sum[2] / kSample, sum[3] / kSample, 0.0};
  double di = 0, dj = 0;
#pragma unroll
  for (int k = 0; k < kSample; ++k) {
    const double ax = x[k][0] - hi.cx, ay = x[k][1] - hi.cy, bx = x[k][2] - hj.cx, by = x[k][3] - hj.cy;
    di += sqrt(ax * ax + ay * ay);
    dj += sqrt(bx * bx + by * by);
  }
  hi.s = sqrt(2.0) / (di / kSample);
  hj.s = sqrt(2.0) / (dj / kSample);
  double A[kSample][9];
#pragma unroll
  for (int k = 0; k < kSample; ++k)
    system_row(hi.s * (x[k][0] - hi.cx), hi.s * (x[k][1] - hi.cy), hj.s * (x[k][2] - hj.cx), hj.s * (x[k][3] - hj.cy),
               A[k]);
  double f[9], F[9];
  null_vector<kSample>(A, f);
  finish_matrix(f, hi, hj, F);
#pragma unroll
  for (int k = 0; k < 9; ++k) Fh[slot * 9 + k] = F[k];
}

// ------------------------------------------------------------------ medians
__global__ __launch_bounds__(kThreads) void k_score(const double* __restrict__ pts,
                                                    const unsigned char* __restrict__ valid, int N, int H,
                                                    const double* __restrict__ Fh, double* __restrict__ med) {
  __shared__ int hist[256];
  __shared__ int pick[2];   // the digit of this pass, the rank inside its bin
  const int h = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const size_t slot = static_cast<size_t>(p) * H + h;
  const double* q = pts + static_cast<size_t>(p) * N * 4;
  const unsigned char* ok = valid ? valid + static_cast<size_t>(p) * N : nullptr;
  double F[9];
  bool usable = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    F[k] = Fh[slot * 9 + k];
    usable &= F[k] == F[k];
  }
  if (!usable) {   // uniform over the block
    if (tid == 0) med[slot] = __longlong_as_double(kInfBits);
    return;
  }
  unsigned long long prefix = 0;
  int rank = 0;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    for (int r = tid; r < N; r += kThreads) {
      if (ok && !ok[r]) continue;
      const unsigned long long bits = error_bits(F, q + static_cast<size_t>(r) * 4);
      // the digits above this pass's; pass 0 has none (a shift by 64 is undefined)
      if (pass == 0 || (bits >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(bits >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid < 64) {
      int c[4], mine = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        c[i] = hist[4 * lane + i];
        mine += c[i];
      }
      int upto = mine;   // inclusive scan over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(upto, o, 64);
        if (lane >= o) upto += t;
      }
      const int total = __shfl(upto, 63, 64);   // read with every lane active
      if (pass == 0) rank = total / 2;          // n / 2: every valid row is in the first histogram
      int r = rank - (upto - mine);
      if (r >= 0 && r < mine) {   // one lane at most; none when there is no valid row
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (r >= 0 && r < c[i]) {
            pick[0] = 4 * lane + i;
            pick[1] = r;
            r = -1;
          } else if (r >= 0) {
            r -= c[i];
          }
        }
      }
      if (lane == 0 && total == 0) pick[0] = -1;
    }
    __syncthreads();
    if (pick[0] < 0) {   // no valid row
      if (tid == 0) med[slot] = __longlong_as_double(kInfBits);
      return;
    }
    prefix |= static_cast<unsigned long long>(pick[0]) << shift;
    rank = pick[1];
    // the next pass's hist[tid] = 0 comes after every thread has read pick: the barrier above orders
    // the histogram reads, and pick is rewritten only after the next pass's two barriers
  }
  if (tid == 0) med[slot] = __longlong_as_double(static_cast<long long>(prefix));
}

// ------------------------------------------------------------------ winner, mask, refit
// F scaled to F[2][2] = 1, or to Frobenius norm 1 when F[2][2] is negligible; false for a zero or
// non-finite matrix
__device__ __forceinline__ bool scale_matrix(double (&F)[9]) {
  double mx = 0, fro = 0;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    mx = fmax(mx, fabs(F[k]));
    fro += F[k] * F[k];
    finite &= fabs(F[k]) <= 1.79769313486231570815e308;
  }
  if (!finite || !(mx > 0.0)) return false;
  const double d = fabs(F[8]) <= 1e-7 * mx ? sqrt(fro) : F[8];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = F[k] / d;
  return true;
}

__global__ __launch_bounds__(kThreads) void k_finalize(const double* __restrict__ pts,
                                                       const unsigned char* __restrict__ valid, int N, int H, int refit,
                                                       const double* __restrict__ Fh, const double* __restrict__ med,
                                                       const int* __restrict__ samples, double* __restrict__ Fout,
                                                       unsigned char* __restrict__ mask, int* __restrict__ sample,
                                                       double* __restrict__ stats) {
  __shared__ double red[45 * kWaves];
  __shared__ double bmed[kThreads];
  __shared__ int bh[kThreads];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* q = pts + static_cast<size_t>(p) * N * 4;
  const unsigned char* ok = valid ? valid + static_cast<size_t>(p) * N : nullptr;
  unsigned char* mk = mask + static_cast<size_t>(p) * N;
  const double inf = __longlong_as_double(kInfBits);

  // the smallest median, ties to the lowest h: each thread over its stride (ascending h), then thread
  // order is not h order, so the final pass compares h as well
  double m = inf;
  int hb = -1;
  for (int h = tid; h < H; h += kThreads) {
    const double v = med[static_cast<size_t>(p) * H + h];
    if (v < m) m = v, hb = h;
  }
  bmed[tid] = m, bh[tid] = hb;
  __syncthreads();
  for (int t = 0; t < kThreads; ++t) {
    const double v = bmed[t];
    const int hv = bh[t];
    if (hv >= 0 && (v < m || (v == m && hv < hb) || hb < 0)) m = v, hb = hv;
  }
  // every thread now holds the same (m, hb); hb < 0: no usable hypothesis

  double nv[1] = {0};
  for (int r = tid; r < N; r += kThreads) nv[0] += (!ok || ok[r]) ? 1.0 : 0.0;
  block_sums<1>(nv, red);
  const int n = static_cast<int>(nv[0]);

  double F[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = hb >= 0 ? Fh[(static_cast<size_t>(p) * H + hb) * 9 + k] : 0.0;
  double sigma = 0;
  if (hb >= 0) {
    const double small = n > 8 ? 5.0 / (n - 8) : 0.0;
    sigma = 2.5 * 1.4826 * (1.0 + small) * sqrt(m);
    sigma = fmax(sigma, kSigmaFloor);
  }
  const double thr = sigma * sigma;

  // inliers of the winner, and the sums of their coordinates
  double s4[5] = {0, 0, 0, 0, 0};
  for (int r = tid; r < N; r += kThreads) {
    bool in = hb >= 0 && (!ok || ok[r]);
    if (in) in = __longlong_as_double(static_cast<long long>(error_bits(F, q + static_cast<size_t>(r) * 4))) <= thr;
    mk[r] = in;
    if (in) {
#pragma unroll
      for (int c = 0; c < 4; ++c) s4[c] += q[static_cast<size_t>(r) * 4 + c];
      s4[4] += 1.0;
    }
  }
  block_sums<5>(s4, red);
  int n_in = static_cast<int>(s4[4]);
  bool good = hb >= 0 && n_in >= kSample;

  if (good && refit) {   // uniform over the block
    Hartley hi = {s4[0] / n_in, s4[1] / n_in, 0.0}, hj = {s4[2] / n_in, s4[3] / n_in, 0.0};
    double d2[2] = {0, 0};
    for (int r = tid; r < N; r += kThreads) {
      if (!mk[r]) continue;   // this thread's own store
      const double* x = q + static_cast<size_t>(r) * 4;
      const double ax = x[0] - hi.cx, ay = x[1] - hi.cy, bx = x[2] - hj.cx, by = x[3] - hj.cy;
      d2[0] += sqrt(ax * ax + ay * ay);
      d2[1] += sqrt(bx * bx + by * by);
    }
    block_sums<2>(d2, red);
    hi.s = sqrt(2.0) / (d2[0] / n_in);
    hj.s = sqrt(2.0) / (d2[1] / n_in);
    double g[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) g[k] = 0;
    for (int r = tid; r < N; r += kThreads) {
      if (!mk[r]) continue;
      const double* x = q + static_cast<size_t>(r) * 4;
      double a[9];
      system_row(hi.s * (x[0] - hi.cx), hi.s * (x[1] - hi.cy), hj.s * (x[2] - hj.cx), hj.s * (x[3] - hj.cy), a);
      int k = 0;
#pragma unroll
      for (int u = 0; u < 9; ++u)
#pragma unroll
        for (int v = u; v < 9; ++v, ++k) g[k] += a[u] * a[v];
    }
    block_sums<45>(g, red);
    if (tid == 0) {
      double G[9][9], f[9];
      int k = 0;
#pragma unroll
      for (int u = 0; u < 9; ++u)
#pragma unroll
        for (int v = u; v < 9; ++v, ++k) G[u][v] = G[v][u] = g[k];
      null_vector<9>(G, f);
      finish_matrix(f, hi, hj, F);
    }
  }
  __syncthreads();   // everyone is done with bh
  if (tid == 0) {
    good = good && scale_matrix(F);
    bh[0] = good;
#pragma unroll
    for (int k = 0; k < 9; ++k) Fout[static_cast<size_t>(p) * 9 + k] = good ? F[k] : 0.0;
#pragma unroll
    for (int k = 0; k < kSample; ++k)
      sample[static_cast<size_t>(p) * kSample + k] =
          hb >= 0 ? samples[(static_cast<size_t>(p) * H + hb) * kSample + k] : -1;
    stats[static_cast<size_t>(p) * 4 + 0] = m;
    stats[static_cast<size_t>(p) * 4 + 1] = sigma;
    stats[static_cast<size_t>(p) * 4 + 2] = good ? n_in : 0;
    stats[static_cast<size_t>(p) * 4 + 3] = hb;
  }
  __syncthreads();
  // a problem that ends without a matrix keeps no inliers
  if (!bh[0])
    for (int r = tid; r < N; r += kThreads) mk[r] = 0;
}

// ------------------------------------------------------------------ the generator's printed check
__global__ __launch_bounds__(kThreads) void k_residual_stats(const double* __restrict__ Fm,
                                                             const double* __restrict__ pts,
                                                             const unsigned char* __restrict__ valid, int N,
                                                             double* __restrict__ out) {
  __shared__ double red[2 * kWaves];
  __shared__ double mx[kWaves];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* q = pts + static_cast<size_t>(p) * N * 4;
  const unsigned char* ok = valid ? valid + static_cast<size_t>(p) * N : nullptr;
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = Fm[static_cast<size_t>(p) * 9 + k];
  double s[2] = {0, 0}, big = 0;
  for (int r = tid; r < N; r += kThreads) {
    if (ok && !ok[r]) continue;
    const double* x = q + static_cast<size_t>(r) * 4;
    const double a = F[0] * x[0] + F[1] * x[1] + F[2], b = F[3] * x[0] + F[4] * x[1] + F[5],
                 c = F[6] * x[0] + F[7] * x[1] + F[8];
    const double e = fabs(x[2] * a + x[3] * b + c);
    s[0] += e;
    s[1] += 1.0;
    big = fmax(big, e);
  }
  big = wave_max(big);
  if ((tid & 63) == 0) mx[tid >> 6] = big;
  block_sums<2>(s, red);   // its barriers also publish mx
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) big = fmax(big, mx[w]);
    out[static_cast<size_t>(p) * 2] = s[1] > 0 ? s[0] / s[1] : 0.0;
    out[static_cast<size_t>(p) * 2 + 1] = big;
  }
}

bool lmeds_shape_ok(int P, int N, int H) {
  return P >= 1 && P <= kMaxProblems && N >= kSample && N <= kMaxRows && H >= 1 && H <= kMaxHypotheses;
}

}  // namespace
}  // namespace posu

using namespace posu;

extern "C" long long posu_fundamental_workspace(int P, int N, int H) {
  if (!lmeds_shape_ok(P, N, H)) return -1;
  // per hypothesis: the matrix (9 f64), its median (f64), its rows (8 i32)
  return static_cast<long long>(P) * H * (9 * 8 + 8 + kSample * 4);
}

extern "C" int posu_fundamental_lmeds(const double* pts, const unsigned char* valid, int P, int N, int H,
                                      unsigned long long seed, int refit, double* F, unsigned char* mask, int* sample,
                                      double* stats, void* workspace, long long workspace_bytes, void* stream) {
  const std::string f("posu_fundamental_lmeds");
  POSU_REQUIRE(P >= 1 && P <= kMaxProblems, f + ": 1 <= P <= 65535 problems expected");
  POSU_REQUIRE(N >= kSample && N <= kMaxRows, f + ": N must be at least 8 rows (and at most 2^26)");
  POSU_REQUIRE(H >= 1 && H <= kMaxHypotheses, f + ": H must be at least 1 hypothesis (and at most 2^20)");
  POSU_REQUIRE(pts && F && mask && sample && stats && workspace, f + ": null pointer");
  POSU_REQUIRE(workspace_bytes >= posu_fundamental_workspace(P, N, H),
               f + ": workspace too small (posu_fundamental_workspace gives the bytes)");
  POSU_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, f + ": workspace must be 8-byte aligned");
  const size_t slots = static_cast<size_t>(P) * H;
  double* Fh = static_cast<double*>(workspace);
  double* med = Fh + slots * 9;
  int* samples = reinterpret_cast<int*>(med + slots);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_hypotheses, dim3((H + kHypLanes - 1) / kHypLanes, P), dim3(kHypLanes), 0, s, pts, valid, N, H,
                     static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), Fh, samples);
  hipLaunchKernelGGL(k_score, dim3(H, P), dim3(kThreads), 0, s, pts, valid, N, H, Fh, med);
  hipLaunchKernelGGL(k_finalize, dim3(P), dim3(kThreads), 0, s, pts, valid, N, H, refit, Fh, med, samples, F, mask,
                     sample, stats);
  return check_launch("posu_fundamental_lmeds");
}

extern "C" int posu_epipolar_residual_stats(const double* F, const double* pts, const unsigned char* valid, int P,
                                            int N, double* out, void* stream) {
  const std::string f("posu_epipolar_residual_stats");
  POSU_REQUIRE(P >= 1 && P <= 0x7fffffff / 16 && N >= 1 && N <= kMaxRows, f + ": bad shape (P >= 1, 1 <= N <= 2^26)");
  POSU_REQUIRE(F && pts && out, f + ": null pointer");
  hipLaunchKernelGGL(k_residual_stats, dim3(P), dim3(kThreads), 0, as_stream(stream), F, pts, valid, N, out);
  return check_launch("posu_epipolar_residual_stats");
}
