// Recursive pictorial structure model (RPSM): multi-view heatmaps -> 3-D pose by max-product
// inference over the skeleton tree on a 3-D bin grid, refined recursively around each joint
// (reference lib/multiviews/pictorial.py; run/test/generate_pairwise_constraints.py for the
// level-1 constraint).  All arithmetic is fp64, no MFMA; parallel over groups, joints / edges
// and bins.
//
// Discrete decisions hang on these floats (inside / outside the heatmap, the limb-length
// tolerance, the argmax), so this file keeps the reference's operation order and is compiled
// without floating-point contraction: a fused multiply-add rounds once where numpy rounds twice.
//
// Kernels:
//   grid_kernel           compute_grid (pictorial.py:108-119): linspace per axis, 'xy' meshgrid order
//   unary_kernel          compute_unary_term (pictorial.py:146-190): project_pose + crop affine +
//                         bilinear sample (scipy RegularGridInterpolator, fill 0), summed over views
//   maxprod_kernel        infer's inner step (pictorial.py:47-59): m_i = max_j P[i,j] e_j and the first
//                         j attaining it; P from a packed bit mask or from the grids on the fly
//                         (compute_pairwise_constrain, pictorial.py:122-143)
//   combine_kernel        E = ((u * m_child1) * m_child2) ... in children order (pictorial.py:58)
//   backtrack_kernel      root argmax + state walk + get_loc_from_cube_idx (pictorial.py:68-105)
//   pairwise_mask_kernel  the packed constraint of all edges from a grid
#pragma clang fp contract(off)
#include "posu_common.h"

namespace posu {
namespace {

constexpr int kMaxJ = 32;
constexpr int kMaxV = 8;
constexpr int kMaxN = 4096;
constexpr int kCam = 20;  // R[9], T[3], f, cx, cy, k[3], p[2]
constexpr int kThreads = 256;
constexpr int kMaxLaunch = 65535;  // grid y / z extent

// by-value launch tables (J <= 32): the launches carry them, no device upload
struct EdgeList {
  int n;
  int parent[kMaxJ];
  int child[kMaxJ];
  int eid[kMaxJ];      // row of the packed mask
  double thr[kMaxJ];   // pairwise_mask_kernel: allowed |d - limb| bound
  double limb[kMaxJ];
};
struct NodeList {
  int n;
  int node[kMaxJ];
  int cbeg[kMaxJ];
  int cend[kMaxJ];
  int cidx[kMaxJ];  // every node's children, in its own order
};
struct Walk {
  int J;
  int root;
  int order[kMaxJ];  // root first, parents before children
  int parent[kMaxJ];
};

// numpy.linspace(-size/2, size/2, n)[i] + c
__device__ __forceinline__ double axis_coord(int i, int n, double size, double c) {
  const double stop = size / 2, start = -size / 2;
  const double step = (stop - start) / static_cast<double>(n - 1);
  const double v = (i == n - 1) ? stop : static_cast<double>(i) * step + start;
  return v + c;
}

// grid [G*NG, N, 3] from centers [G*NG, 3]; flat bin b = (a*n + bx)*n + c -> (x[bx], y[a], z[c])
__global__ __launch_bounds__(kThreads) void grid_kernel(const double* __restrict__ centers, int n, int N,
                                                        double size, double* __restrict__ grid) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= N) return;
  const size_t q = blockIdx.y;
  const double* c = centers + q * 3;
  const int iz = b % n, ix = (b / n) % n, iy = b / (n * n);
  double* o = grid + (q * N + b) * 3;
  o[0] = axis_coord(ix, n, size, c[0]);
  o[1] = axis_coord(iy, n, size, c[1]);
  o[2] = axis_coord(iz, n, size, c[2]);
}

// cell index of scipy's find_indices on the grid 0..n-1: floor(x) clipped to [0, n-2]
__device__ __forceinline__ int cell_of(double x, int n) {
  const double f = floor(x);
  int i = (f >= static_cast<double>(n - 2)) ? n - 2 : ((f > 0.0) ? static_cast<int>(f) : 0);
  return i;
}

__global__ __launch_bounds__(kThreads) void unary_kernel(const float* __restrict__ hm,
                                                         const double* __restrict__ cams,
                                                         const double* __restrict__ affine,
                                                         const double* __restrict__ grid, int NG, int V, int J,
                                                         int H, int N, double img_w, double img_h,
                                                         double* __restrict__ unary) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= N) return;
  const int j = blockIdx.y, g = blockIdx.z;
  const double* x = grid + ((static_cast<size_t>(g) * NG + (NG == 1 ? 0 : j)) * N + b) * 3;
  const double X = x[0], Y = x[1], Z = x[2];
  const double hsz = static_cast<double>(H), top = static_cast<double>(H - 1);
  double acc = 0.0;
  for (int v = 0; v < V; ++v) {
    const double* c = cams + (static_cast<size_t>(g) * V + v) * kCam;
    // project_point_radial (cameras.py:38-49), avg_f
    const double d0 = X - c[9], d1 = Y - c[10], d2 = Z - c[11];
    const double xc0 = (c[0] * d0 + c[1] * d1) + c[2] * d2;
    const double xc1 = (c[3] * d0 + c[4] * d1) + c[5] * d2;
    const double xc2 = (c[6] * d0 + c[7] * d1) + c[8] * d2;
    const double y0 = xc0 / xc2, y1 = xc1 / xc2;
    const double r2 = y0 * y0 + y1 * y1;
    const double radial = 1.0 + ((c[15] * r2 + c[16] * (r2 * r2)) + c[17] * (r2 * r2 * r2));
    const double tan = c[18] * y1 + c[19] * y0;
    const double s = radial + tan;
    const double u0 = y0 * s + c[19] * r2, u1 = y1 * s + c[18] * r2;
    const double px = c[12] * u0 + c[13], py = c[12] * u1 + c[14];
    // affine_transform, then * [w, h] / image_size (pictorial.py:174)
    const double* a = affine + (static_cast<size_t>(g) * V + v) * 6;
    const double qx = ((a[0] * px + a[1] * py) + a[2]) * hsz / img_w;
    const double qy = ((a[3] * px + a[4] * py) + a[5]) * hsz / img_h;
    // RegularGridInterpolator(points = [0..h-1, 0..w-1], values = hmap.T, linear, fill_value = 0)
    const bool out = qx < 0.0 || qx > top || qy < 0.0 || qy > top;
    const int i0 = cell_of(qx, H), i1 = cell_of(qy, H);
    const double t0 = qx - static_cast<double>(i0), t1 = qy - static_cast<double>(i1);
    const double s0 = 1.0 - t0, s1 = 1.0 - t1;
    const float* m = hm + ((static_cast<size_t>(g) * V + v) * J + j) * H * H;
    const double f00 = m[i1 * H + i0], f01 = m[(i1 + 1) * H + i0];
    const double f10 = m[i1 * H + i0 + 1], f11 = m[(i1 + 1) * H + i0 + 1];
    double val = 0.0 + f00 * (s0 * s1);
    val = val + f01 * (s0 * t1);
    val = val + f10 * (t0 * s1);
    val = val + f11 * (t0 * t1);
    acc = acc + (out ? 0.0 : val);
  }
  unary[(static_cast<size_t>(g) * J + j) * N + b] = acc;
}

// One (group, edge) and a block of parent bins per workgroup.  The child's energies sit in LDS;
// every lane owns one parent bin and walks j upwards, so the strict `>` keeps the first maximum
// (numpy.argmax) with no cross-lane reduction.  v_j = P[i,j] * e_j: a disallowed pair gives a
// (signed) zero, not -inf.  FLY: P from the grids, |norm(g_p[i] - g_c[j]) - limbs[g][child]| <= tol.
template <bool FLY>
__global__ __launch_bounds__(kThreads) void maxprod_kernel(const double* __restrict__ energy,
                                                           const uint32_t* __restrict__ mask,
                                                           const double* __restrict__ grid, int NG,
                                                           const double* __restrict__ limbs, double tol,
                                                           EdgeList ed, int J, int N, double* __restrict__ maxv,
                                                           int* __restrict__ state) {
  __shared__ double e[kMaxN];
  const int k = blockIdx.y, g = blockIdx.z;
  const int child = ed.child[k], parent = ed.parent[k];
  const double* ce = energy + (static_cast<size_t>(g) * J + child) * N;
  for (int j = threadIdx.x; j < N; j += kThreads) e[j] = ce[j];
  __syncthreads();
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  double best;
  int arg = 0;
  if (FLY) {
    const double* gp = grid + ((static_cast<size_t>(g) * NG + (NG == 1 ? 0 : parent)) * N + i) * 3;
    const double* gc = grid + (static_cast<size_t>(g) * NG + (NG == 1 ? 0 : child)) * N * 3;
    const double px = gp[0], py = gp[1], pz = gp[2], limb = limbs[static_cast<size_t>(g) * J + child];
    best = 0.0;
    for (int j = 0; j < N; ++j) {
      const double dx = px - gc[3 * j], dy = py - gc[3 * j + 1], dz = pz - gc[3 * j + 2];
      const double len = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
      const double v = (fabs(len - limb) <= tol) ? e[j] : 0.0 * e[j];
      if (j == 0 || v > best) {
        best = v;
        arg = j;
      }
    }
  } else {
    const int Wd = (N + 31) >> 5;
    // word w of parent bin i at [edge][w][i]: consecutive lanes read consecutive words
    const uint32_t* col = mask + static_cast<size_t>(ed.eid[k]) * Wd * N + i;
    best = (col[0] & 1u) ? e[0] : 0.0 * e[0];
    for (int w = 0; w < Wd; ++w) {
      const uint32_t bits = col[static_cast<size_t>(w) * N];
      const int j0 = w << 5;
      if (bits == 0u) {
        // 32 disallowed pairs: all zeros, only the first can beat a negative maximum
        const double v = 0.0 * e[j0];
        if (v > best) {
          best = v;
          arg = j0;
        }
        continue;
      }
      const int nb = min(32, N - j0);
      for (int t = 0; t < nb; ++t) {
        const double ej = e[j0 + t];
        const double v = ((bits >> t) & 1u) ? ej : 0.0 * ej;
        if (v > best) {
          best = v;
          arg = j0 + t;
        }
      }
    }
  }
  const size_t o = (static_cast<size_t>(g) * J + child) * N + i;
  maxv[o] = best;
  state[o] = arg;
}

__global__ __launch_bounds__(kThreads) void combine_kernel(const double* __restrict__ unary,
                                                           const double* __restrict__ maxv, NodeList nl, int J,
                                                           int N, double* __restrict__ energy) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int k = blockIdx.y;
  const size_t base = static_cast<size_t>(blockIdx.z) * J;
  double v = unary[(base + nl.node[k]) * N + i];
  for (int c = nl.cbeg[k]; c < nl.cend[k]; ++c) v = v * maxv[(base + nl.cidx[c]) * N + i];
  energy[(base + nl.node[k]) * N + i] = v;
}

// One workgroup per group: first argmax of the root's energy, then every joint takes
// state[joint][its parent's bin]; pose = the chosen bins' grid coordinates.
__global__ __launch_bounds__(kThreads) void backtrack_kernel(const double* __restrict__ energy,
                                                             const int* __restrict__ state,
                                                             const double* __restrict__ grid, int NG, Walk wk,
                                                             int N, int* __restrict__ bins,
                                                             double* __restrict__ pose,
                                                             double* __restrict__ pose_copy) {
  __shared__ double sv[kThreads];
  __shared__ int si[kThreads];
  __shared__ int sb[kMaxJ];
  const int g = blockIdx.x, J = wk.J, tid = threadIdx.x;
  const double* er = energy + (static_cast<size_t>(g) * J + wk.root) * N;
  double best = -INFINITY;
  int arg = 0x7fffffff;
  if (tid < N) {
    best = er[tid];
    arg = tid;
  }
  for (int i = tid + kThreads; i < N; i += kThreads) {
    const double v = er[i];
    if (v > best) {
      best = v;
      arg = i;
    }
  }
  sv[tid] = best;
  si[tid] = arg;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double v = sv[tid + s];
      const int a = si[tid + s];
      if (v > sv[tid] || (v == sv[tid] && a < si[tid])) {
        sv[tid] = v;
        si[tid] = a;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    sb[wk.root] = min(max(si[0], 0), N - 1);
    for (int k = 1; k < J; ++k) {
      const int c = wk.order[k];
      const int s = state[(static_cast<size_t>(g) * J + c) * N + sb[wk.parent[c]]];
      sb[c] = min(max(s, 0), N - 1);
    }
  }
  __syncthreads();
  if (tid < J && bins) bins[g * J + tid] = sb[tid];
  if (tid < J * 3 && (pose || pose_copy)) {
    const int j = tid / 3, a = tid - j * 3;
    const double v = grid[((static_cast<size_t>(g) * NG + (NG == 1 ? 0 : j)) * N + sb[j]) * 3 + a];
    const size_t o = (static_cast<size_t>(g) * J + j) * 3 + a;
    if (pose) pose[o] = v;
    if (pose_copy) pose_copy[o] = v;
  }
}

// mask [E, ceil(N/32), N]: bit j & 31 of word [e][j / 32][i] = |norm(g_p[i] - g_c[j]) - limb| (< | <=) thr
__global__ __launch_bounds__(kThreads) void pairwise_mask_kernel(const double* __restrict__ grid, int NG,
                                                                 int N, EdgeList ed, int strict,
                                                                 uint32_t* __restrict__ mask) {
  const int Wd = (N + 31) >> 5;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= N * Wd) return;
  const int k = blockIdx.y, w = t / N, i = t - w * N;
  const double* gp = grid + (static_cast<size_t>(NG == 1 ? 0 : ed.parent[k]) * N + i) * 3;
  const double* gc = grid + static_cast<size_t>(NG == 1 ? 0 : ed.child[k]) * N * 3;
  const double px = gp[0], py = gp[1], pz = gp[2], limb = ed.limb[k], thr = ed.thr[k];
  uint32_t bits = 0;
  const int j0 = w << 5, nb = min(32, N - j0);
  for (int b = 0; b < nb; ++b) {
    const int j = j0 + b;
    const double dx = px - gc[3 * j], dy = py - gc[3 * j + 1], dz = pz - gc[3 * j + 2];
    const double off = fabs(__dsqrt_rn((dx * dx + dy * dy) + dz * dz) - limb);
    if (strict ? (off < thr) : (off <= thr)) bits |= 1u << b;
  }
  mask[(static_cast<size_t>(ed.eid[k]) * Wd + w) * N + i] = bits;
}

// ---- host: the tree
struct Tree {
  int J = 0, root = -1, maxdepth = 0;
  int parent[kMaxJ], cptr[kMaxJ + 1], cidx[kMaxJ], eid[kMaxJ], depth[kMaxJ], order[kMaxJ];
};

// parent [J] (root = -1), child_ptr [J + 1], child_idx [J - 1]: node n's ordered children are
// child_idx[child_ptr[n] .. child_ptr[n + 1]); edge e of the packed mask is child_idx[e]'s edge.
const char* read_tree(const int* parent, const int* child_ptr, const int* child_idx, int J, Tree& t) {
  t.J = J;
  for (int j = 0; j < J; ++j) {
    if (parent[j] == -1) {
      if (t.root != -1) return "more than one root";
      t.root = j;
    } else if (parent[j] < 0 || parent[j] >= J || parent[j] == j) {
      return "parent out of range";
    }
    t.parent[j] = parent[j];
    t.eid[j] = -1;
  }
  if (t.root < 0) return "no root (parent == -1)";
  if (child_ptr[0] != 0 || child_ptr[J] != J - 1) return "child_ptr must run from 0 to J - 1";
  for (int j = 0; j < J; ++j) {
    if (child_ptr[j + 1] < child_ptr[j]) return "child_ptr must not decrease";
    t.cptr[j] = child_ptr[j];
    for (int e = child_ptr[j]; e < child_ptr[j + 1]; ++e) {
      const int c = child_idx[e];
      if (c < 0 || c >= J || parent[c] != j || t.eid[c] != -1) return "children do not match the parent array";
      t.cidx[e] = c;
      t.eid[c] = e;
    }
  }
  t.cptr[J] = J - 1;
  // breadth-first order; a cycle leaves joints unreached
  int head = 0, tail = 0;
  t.order[tail++] = t.root;
  t.depth[t.root] = 0;
  while (head < tail) {
    const int n = t.order[head++];
    for (int e = t.cptr[n]; e < t.cptr[n + 1]; ++e) {
      t.depth[t.cidx[e]] = t.depth[n] + 1;
      t.maxdepth = std::max(t.maxdepth, t.depth[n] + 1);
      t.order[tail++] = t.cidx[e];
    }
  }
  if (tail != J) return "the parent array is not a tree";
  return nullptr;
}

inline int blocks_of(int n) { return (n + kThreads - 1) / kThreads; }

int launch_grid(const double* centers, int count, double size, int nbins, double* grid, hipStream_t s) {
  const int N = nbins * nbins * nbins;
  if (count == 0) return POSU_OK;
  grid_kernel<<<dim3(blocks_of(N), count), kThreads, 0, s>>>(centers, nbins, N, size, grid);
  return check_launch("posu_rpsm_grid");
}

int launch_unary(const float* hm, const double* cams, const double* affine, int G, int V, int J, int H,
                 double img_w, double img_h, const double* grid, int NG, int N, double* unary, hipStream_t s) {
  if (G == 0) return POSU_OK;
  unary_kernel<<<dim3(blocks_of(N), J, G), kThreads, 0, s>>>(hm, cams, affine, grid, NG, V, J, H, N, img_w,
                                                             img_h, unary);
  return check_launch("posu_rpsm_unary");
}

// one max-product + one combine launch per tree depth, deepest first
int launch_infer(const Tree& t, const double* unary, const uint32_t* mask, const double* grid, int NG,
                 const double* limb, double tol, int G, int N, double* energy, double* maxv, int* state,
                 hipStream_t s) {
  if (G == 0) return POSU_OK;
  const int J = t.J;
  for (int d = t.maxdepth; d >= 0; --d) {
    EdgeList ed;
    NodeList nl;
    ed.n = nl.n = 0;
    for (int e = 0; e < J - 1; ++e) nl.cidx[e] = t.cidx[e];
    for (int j = 0; j < J; ++j) {
      if (t.depth[j] != d) continue;
      nl.node[nl.n] = j;
      nl.cbeg[nl.n] = t.cptr[j];
      nl.cend[nl.n] = t.cptr[j + 1];
      ++nl.n;
      for (int e = t.cptr[j]; e < t.cptr[j + 1]; ++e) {
        const int c = t.cidx[e];
        ed.parent[ed.n] = j;
        ed.child[ed.n] = c;
        ed.eid[ed.n] = e;
        ed.limb[ed.n] = 0.0;
        ed.thr[ed.n] = tol;
        ++ed.n;
      }
    }
    if (ed.n > 0) {
      const dim3 gr(blocks_of(N), ed.n, G);
      if (mask)
        maxprod_kernel<false><<<gr, kThreads, 0, s>>>(energy, mask, nullptr, 1, nullptr, 0.0, ed, J, N, maxv, state);
      else
        maxprod_kernel<true><<<gr, kThreads, 0, s>>>(energy, nullptr, grid, NG, limb, tol, ed, J, N, maxv, state);
      if (int st = check_launch("posu_rpsm_infer (max-product)")) return st;
    }
    combine_kernel<<<dim3(blocks_of(N), nl.n, G), kThreads, 0, s>>>(unary, maxv, nl, J, N, energy);
    if (int st = check_launch("posu_rpsm_infer (combine)")) return st;
  }
  return POSU_OK;
}

int launch_backtrack(const Tree& t, const double* energy, const int* state, const double* grid, int NG, int G,
                     int N, int* bins, double* pose, double* pose_copy, hipStream_t s) {
  if (G == 0) return POSU_OK;
  Walk wk;
  wk.J = t.J;
  wk.root = t.root;
  for (int j = 0; j < t.J; ++j) {
    wk.order[j] = t.order[j];
    wk.parent[j] = t.parent[j];
  }
  backtrack_kernel<<<G, kThreads, 0, s>>>(energy, state, grid, NG, wk, N, bins, pose, pose_copy);
  return check_launch("posu_rpsm_backtrack");
}

inline long long align256(long long b) { return (b + 255) / 256 * 256; }

struct Workspace {
  double *grid, *unary, *energy, *maxv, *pose;
  int *state, *bins;
  long long bytes;
};

Workspace carve(void* base, int G, int J, int Nmax) {
  Workspace w;
  char* p = static_cast<char*>(base);
  long long o = 0;
  const long long gjn = static_cast<long long>(G) * J * Nmax;
  auto take = [&](long long bytes) {
    char* r = p ? p + o : nullptr;
    o += align256(bytes);
    return r;
  };
  w.grid = reinterpret_cast<double*>(take(gjn * 3 * 8));
  w.unary = reinterpret_cast<double*>(take(gjn * 8));
  w.energy = reinterpret_cast<double*>(take(gjn * 8));
  w.maxv = reinterpret_cast<double*>(take(gjn * 8));
  w.pose = reinterpret_cast<double*>(take(static_cast<long long>(G) * J * 3 * 8));
  w.state = reinterpret_cast<int*>(take(gjn * 4));
  w.bins = reinterpret_cast<int*>(take(static_cast<long long>(G) * J * 4));
  w.bytes = o;
  return w;
}

inline bool cube_ok(int nbins) { return nbins >= 2 && nbins <= 16; }  // 16^3 = kMaxN

}  // namespace
}  // namespace posu

using namespace posu;

#define RPSM_TREE(name)                                                                        \
  POSU_REQUIRE(parent && child_ptr && child_idx, name ": null pointer (tree)");               \
  Tree tree;                                                                                   \
  if (const char* why = read_tree(parent, child_ptr, child_idx, J, tree)) {                    \
    set_error(std::string(name ": bad tree: ") + why);                                         \
    return POSU_ERR_ARG;                                                                       \
  }

extern "C" long long posu_rpsm_workspace_bytes(int G, int J, int first_nbins, int recur_nbins) {
  if (G < 0 || J < 2 || J > kMaxJ || !cube_ok(first_nbins) || !cube_ok(recur_nbins)) return -1;
  const int n = std::max(first_nbins, recur_nbins);
  return carve(nullptr, G, J, n * n * n).bytes;
}

extern "C" int posu_rpsm_grid(const double* centers, int count, double size, int nbins, double* grid,
                              void* stream) {
  POSU_REQUIRE(centers && grid, "posu_rpsm_grid: null pointer");
  POSU_REQUIRE(count >= 0 && count <= kMaxLaunch, "posu_rpsm_grid: 0 <= grid count <= 65535");
  POSU_REQUIRE(nbins >= 2, "posu_rpsm_grid: nbins >= 2 (linspace needs two points)");
  POSU_REQUIRE(nbins <= 16, "posu_rpsm_grid: N = nbins^3 <= 4096");
  return launch_grid(centers, count, size, nbins, grid, as_stream(stream));
}

extern "C" int posu_rpsm_unary(const float* heatmaps, const double* cams, const double* affine, int G, int V,
                               int J, int H, int W, double img_w, double img_h, const double* grid, int NG,
                               int N, double* unary, void* stream) {
  POSU_REQUIRE(heatmaps && cams && affine && grid && unary, "posu_rpsm_unary: null pointer");
  POSU_REQUIRE(G >= 0 && G <= kMaxLaunch, "posu_rpsm_unary: 0 <= G <= 65535");
  POSU_REQUIRE(V >= 1 && V <= kMaxV, "posu_rpsm_unary: 1 <= V <= 8");
  POSU_REQUIRE(J >= 2 && J <= kMaxJ, "posu_rpsm_unary: 2 <= J <= 32");
  POSU_REQUIRE(H == W, "posu_rpsm_unary: H == W (the reference's interpolator swaps the axes' sizes, so it "
                       "only works for square heatmaps)");
  POSU_REQUIRE(H >= 2, "posu_rpsm_unary: heatmaps of at least 2 x 2");
  POSU_REQUIRE(N >= 1 && N <= kMaxN, "posu_rpsm_unary: 1 <= N <= 4096");
  POSU_REQUIRE(NG == 1 || NG == J, "posu_rpsm_unary: one grid per group or one per joint");
  return launch_unary(heatmaps, cams, affine, G, V, J, H, img_w, img_h, grid, NG, N, unary, as_stream(stream));
}

extern "C" int posu_rpsm_infer(const double* unary, const int* parent, const int* child_ptr,
                               const int* child_idx, const unsigned int* mask, const double* grid, int NG,
                               const double* limb, double tolerance, int G, int J, int N, double* energy,
                               double* maxv, int* state, void* stream) {
  POSU_REQUIRE(unary && energy && maxv && state, "posu_rpsm_infer: null pointer");
  POSU_REQUIRE(J >= 2 && J <= kMaxJ, "posu_rpsm_infer: 2 <= J <= 32");
  POSU_REQUIRE(G >= 0 && G <= kMaxLaunch, "posu_rpsm_infer: 0 <= G <= 65535");
  POSU_REQUIRE(N >= 1 && N <= kMaxN, "posu_rpsm_infer: 1 <= N <= 4096");
  POSU_REQUIRE(mask || (grid && limb), "posu_rpsm_infer: null pointer (a packed mask, or grids and limb lengths)");
  POSU_REQUIRE(mask || NG == 1 || NG == J, "posu_rpsm_infer: one grid per group or one per joint");
  RPSM_TREE("posu_rpsm_infer");
  return launch_infer(tree, unary, mask, grid, NG, limb, tolerance, G, N, energy, maxv, state, as_stream(stream));
}

extern "C" int posu_rpsm_backtrack(const double* energy, const int* state, const int* parent,
                                   const int* child_ptr, const int* child_idx, const double* grid, int NG, int G,
                                   int J, int N, int* bins, double* pose, void* stream) {
  POSU_REQUIRE(energy && state && (bins || pose) && (grid || !pose), "posu_rpsm_backtrack: null pointer");
  POSU_REQUIRE(J >= 2 && J <= kMaxJ, "posu_rpsm_backtrack: 2 <= J <= 32");
  POSU_REQUIRE(G >= 0 && N >= 1 && N <= kMaxN, "posu_rpsm_backtrack: 1 <= N <= 4096");
  POSU_REQUIRE(!pose || NG == 1 || NG == J, "posu_rpsm_backtrack: one grid per group or one per joint");
  RPSM_TREE("posu_rpsm_backtrack");
  return launch_backtrack(tree, energy, state, grid, NG, G, N, bins, pose, nullptr, as_stream(stream));
}

extern "C" int posu_rpsm_pairwise_mask(const double* grid, int NG, int N, const int* parent, const int* child_ptr,
                                       const int* child_idx, int J, const double* limb, const double* thr,
                                       int strict, unsigned int* mask, void* stream) {
  POSU_REQUIRE(grid && limb && thr && mask, "posu_rpsm_pairwise_mask: null pointer");
  POSU_REQUIRE(J >= 2 && J <= kMaxJ, "posu_rpsm_pairwise_mask: 2 <= J <= 32");
  POSU_REQUIRE(N >= 1 && N <= kMaxN, "posu_rpsm_pairwise_mask: 1 <= N <= 4096");
  POSU_REQUIRE(NG == 1 || NG == J, "posu_rpsm_pairwise_mask: one grid, or one per joint");
  RPSM_TREE("posu_rpsm_pairwise_mask");
  EdgeList ed;
  ed.n = J - 1;
  for (int e = 0; e < J - 1; ++e) {
    const int c = tree.cidx[e];
    ed.parent[e] = tree.parent[c];
    ed.child[e] = c;
    ed.eid[e] = e;
    ed.limb[e] = limb[c];
    ed.thr[e] = thr[c];
  }
  const int Wd = (N + 31) / 32;
  pairwise_mask_kernel<<<dim3(blocks_of(N * Wd), J - 1), kThreads, 0, as_stream(stream)>>>(grid, NG, N, ed,
                                                                                         strict, mask);
  return check_launch("posu_rpsm_pairwise_mask");
}

extern "C" int posu_rpsm_run(const float* heatmaps, const double* cams, const double* affine, int G, int V,
                             int J, int H, int W, double img_w, double img_h, const double* grid_centers,
                             double grid_size, int first_nbins, int recur_nbins, int recur_depth,
                             double tolerance, const double* limb, const unsigned int* mask, const int* parent,
                             const int* child_ptr, const int* child_idx, void* workspace,
                             long long workspace_bytes, double* pose, double* level_poses, void* stream) {
  POSU_REQUIRE(heatmaps && cams && affine && grid_centers && limb && mask && workspace && pose,
               "posu_rpsm_run: null pointer");
  POSU_REQUIRE(V >= 1 && V <= kMaxV, "posu_rpsm_run: 1 <= V <= 8");
  POSU_REQUIRE(J >= 2 && J <= kMaxJ, "posu_rpsm_run: 2 <= J <= 32");
  POSU_REQUIRE(G >= 0 && G <= kMaxLaunch / J, "posu_rpsm_run: 0 <= G * J <= 65535 (split larger batches)");
  POSU_REQUIRE(H == W, "posu_rpsm_run: H == W (the reference's interpolator swaps the axes' sizes, so it only "
                       "works for square heatmaps)");
  POSU_REQUIRE(H >= 2, "posu_rpsm_run: heatmaps of at least 2 x 2");
  POSU_REQUIRE(first_nbins >= 2 && recur_nbins >= 2, "posu_rpsm_run: nbins >= 2");
  POSU_REQUIRE(first_nbins <= 16 && recur_nbins <= 16, "posu_rpsm_run: N = nbins^3 <= 4096");
  POSU_REQUIRE(recur_depth >= 0, "posu_rpsm_run: negative recursion depth");
  RPSM_TREE("posu_rpsm_run");
  const int N1 = first_nbins * first_nbins * first_nbins, Nr = recur_nbins * recur_nbins * recur_nbins;
  const Workspace ws = carve(workspace, G, J, std::max(N1, Nr));
  POSU_REQUIRE(workspace_bytes >= ws.bytes, "posu_rpsm_run: workspace smaller than posu_rpsm_workspace_bytes");
  hipStream_t s = as_stream(stream);
  const size_t pose_elems = static_cast<size_t>(G) * J * 3;
  int st;
  // level 1: one grid per group, the caller's packed constraint (pictorial.py:236-241)
  if ((st = launch_grid(grid_centers, G, grid_size, first_nbins, ws.grid, s))) return st;
  if ((st = launch_unary(heatmaps, cams, affine, G, V, J, H, img_w, img_h, ws.grid, 1, N1, ws.unary, s))) return st;
  if ((st = launch_infer(tree, ws.unary, mask, nullptr, 1, nullptr, 0.0, G, N1, ws.energy, ws.maxv, ws.state, s)))
    return st;
  if ((st = launch_backtrack(tree, ws.energy, ws.state, ws.grid, 1, G, N1, ws.bins, ws.pose, level_poses, s)))
    return st;
  // refinements: a grid per joint around its estimate, constraint from the grids (pictorial.py:243-248)
  double cur = grid_size / first_nbins;
  for (int d = 0; d < recur_depth; ++d) {
    if ((st = launch_grid(ws.pose, G * J, cur, recur_nbins, ws.grid, s))) return st;
    if ((st = launch_unary(heatmaps, cams, affine, G, V, J, H, img_w, img_h, ws.grid, J, Nr, ws.unary, s))) return st;
    if ((st = launch_infer(tree, ws.unary, nullptr, ws.grid, J, limb, tolerance, G, Nr, ws.energy, ws.maxv,
                           ws.state, s)))
      return st;
    double* copy = level_poses ? level_poses + (d + 1) * pose_elems : nullptr;
    if ((st = launch_backtrack(tree, ws.energy, ws.state, ws.grid, J, G, Nr, ws.bins, ws.pose, copy, s))) return st;
    cur = cur / recur_nbins;
  }
  if (G > 0 && hipMemcpyAsync(pose, ws.pose, pose_elems * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    set_error("posu_rpsm_run: device copy of the pose failed");
    return POSU_ERR_HIP;
  }
  return POSU_OK;
}
