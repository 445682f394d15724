// Running statistics of the device-resident solution: per-node weighted means and central second moments (mean
// velocity, Reynolds stresses, scalar variance and flux, pressure variance), their reduction over groups of nodes
// (profiles along lines / planes of constant coordinate) and the read-out of one quantity.
//
// Replaces what a driver would do with a get_state copy after every step and numpy sums on the host.  The update is a
// pure stream over nodal vectors that already sit in HBM: ONE launch per sample reads the sample and reads and writes
// every accumulator once.
//
// Layout (nsfem_internal.hpp): one array per quantity, array q of a field at acc + q * stride with stride even, so a
// thread that owns the nodes 2 i and 2 i + 1 moves 16 bytes per access everywhere -- the node-interleaved velocity
// pair is 2 (2D) or 3 (3D) such loads, each accumulator one load and one store.
//
// Update with a = w / (W + w), b = w W / (W + w) (host doubles):
//   d_i = x_i - m_i;   m_i += a d_i;   C_ij += b d_i d_j        (every d taken before a mean moves)
// elementwise, no atomics, no LDS.  The profile kernel folds its sums as k_vol_functionals does: a thread adds its
// nodes in ascending list order, a wave folds its lanes with a fixed xor-shuffle tree, the 4 waves are added in wave
// order (block_sum_all, element_front.hpp).  Same samples, same bytes.
#include "element_front.hpp"

namespace nsfem {

// columns of the accumulators of a field with DIM velocity-like variables (+ the scalar): see stats_columns
template <int DIM, bool SCALAR>
struct StatsCols {
  static constexpr int NCOV = DIM * (DIM + 1) / 2;
  static constexpr int NV = DIM + (SCALAR ? 1 : 0);              // variables: u_0 .. u_{DIM-1}, T
  static constexpr int NQ = DIM + NCOV + (SCALAR ? 2 + DIM : 0);
  static constexpr int NM = NQ - NV;                             // second-moment columns
  __host__ __device__ static constexpr int mean(int v) { return v < DIM ? v : DIM + NCOV; }
};

// W doubles moved as one access
template <int W> struct Lanes { double v[W]; };
template <> struct alignas(16) Lanes<2> { double v[2]; };

// f(c, k, i, j) for every second-moment column c = <d_i d_j>, in column order; k = 0, 1, ... counts them
template <int DIM, bool SCALAR, class F>
__device__ __forceinline__ void stats_for_each_pair(F&& f) {
  using L = StatsCols<DIM, SCALAR>;
  int c = DIM, k = 0;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = i; j < DIM; ++j) f(c++, k++, i, j);
  if constexpr (SCALAR) {
    f(DIM + L::NCOV + 1, L::NCOV, DIM, DIM);
#pragma unroll
    for (int i = 0; i < DIM; ++i) f(DIM + L::NCOV + 2 + i, L::NCOV + 1 + i, i, DIM);
  }
}

// the W consecutive nodes from `node` on (node even for W = 2): all columns loaded, updated, stored
template <int DIM, bool SCALAR, int W>
__device__ __forceinline__ void stats_update_nodes(double* __restrict__ acc, size_t stride, size_t node,
                                                   const double (&x)[DIM + (SCALAR ? 1 : 0)][W], double a, double b,
                                                   int first) {
  using L = StatsCols<DIM, SCALAR>;
  Lanes<W> q[L::NQ];
#pragma unroll
  for (int c = 0; c < L::NQ; ++c) q[c] = *reinterpret_cast<const Lanes<W>*>(acc + (size_t)c * stride + node);
  double d[L::NV][W];
#pragma unroll
  for (int v = 0; v < L::NV; ++v)
#pragma unroll
    for (int l = 0; l < W; ++l) {
      double& m = q[L::mean(v)].v[l];
      d[v][l] = x[v][l] - m;
      // d == 0 keeps the mean's bytes (-0.0 + a * 0.0 would be +0.0): an unchanged field stays bit for bit
      m = first ? x[v][l] : d[v][l] == 0.0 ? m : m + a * d[v][l];
    }
  stats_for_each_pair<DIM, SCALAR>([&](int c, int, int i, int j) {
#pragma unroll
    for (int l = 0; l < W; ++l) q[c].v[l] += (b * d[i][l]) * d[j][l];
  });
#pragma unroll
  for (int c = 0; c < L::NQ; ++c) *reinterpret_cast<Lanes<W>*>(acc + (size_t)c * stride + node) = q[c];
}

// the sample of the W nodes from `node` on: x[v][l]; u node-interleaved [n][DIM], T [n]
template <int DIM, bool SCALAR, int W>
__device__ __forceinline__ void stats_load_sample(const double* __restrict__ u, const double* __restrict__ T,
                                                  size_t node, double (&x)[DIM + (SCALAR ? 1 : 0)][W]) {
  if constexpr (W == 2) {
    // DIM * 2 doubles from u + DIM * node (node even: 16-byte aligned) as DIM 16-byte loads
    Lanes<2> r[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) r[k] = reinterpret_cast<const Lanes<2>*>(u + (size_t)DIM * node)[k];
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int v = 0; v < DIM; ++v) x[v][l] = r[(l * DIM + v) / 2].v[(l * DIM + v) % 2];
    if constexpr (SCALAR) {
      const Lanes<2> t = *reinterpret_cast<const Lanes<2>*>(T + node);
      x[DIM][0] = t.v[0];
      x[DIM][1] = t.v[1];
    }
  } else {
#pragma unroll
    for (int v = 0; v < DIM; ++v) x[v][0] = u[(size_t)DIM * node + v];
    if constexpr (SCALAR) x[DIM][0] = T[node];
  }
}

// n nodes of one field: pairs of nodes grid-strided over `blocks` workgroups, the odd last node on its own
template <int DIM, bool SCALAR>
__device__ __forceinline__ void stats_update_field(int block, int blocks, int64_t n, const double* __restrict__ u,
                                                   const double* __restrict__ T, double* __restrict__ acc,
                                                   size_t stride, double a, double b, int first) {
  constexpr int NV = DIM + (SCALAR ? 1 : 0);
  const int64_t items = (n + 1) / 2;
  for (int64_t i = (int64_t)block * blockDim.x + threadIdx.x; i < items; i += (int64_t)blocks * blockDim.x) {
    const size_t node = 2 * (size_t)i;
    if ((int64_t)node + 1 < n) {
      double x[NV][2];
      stats_load_sample<DIM, SCALAR, 2>(u, T, node, x);
      stats_update_nodes<DIM, SCALAR, 2>(acc, stride, node, x, a, b, first);
    } else {   // (2 n + 1)^d lattice nodes: the count is odd
      double x[NV][1];
      stats_load_sample<DIM, SCALAR, 1>(u, T, node, x);
      stats_update_nodes<DIM, SCALAR, 1>(acc, stride, node, x, a, b, first);
    }
  }
}

template <int DIM, bool SCALAR>
__global__ __launch_bounds__(256) void k_stats_update(StatsUpdate A) {
  const int blk = (int)blockIdx.x;
  if (blk < A.blocks2)
    stats_update_field<DIM, SCALAR>(blk, A.blocks2, A.n2, A.u, A.T, A.acc2, A.stride2, A.a, A.b, A.first);
  else   // the pressure: one variable, its mean and its variance
    stats_update_field<1, false>(blk - A.blocks2, (int)gridDim.x - A.blocks2, A.n1, A.p, nullptr, A.acc1, A.stride1,
                                 A.a, A.b, A.first);
}

// at most this many workgroups per field, the rest grid-strided (a memory-bound stream)
constexpr int kStatsBlocks2 = 2048, kStatsBlocks1 = 512;

void launch_stats_update(hipStream_t s, int dim, bool scalar, StatsUpdate a) {
  auto blocks = [](int64_t n, int cap) { return (int)std::min<int64_t>(((n + 1) / 2 + 255) / 256, cap); };
  a.blocks2 = blocks(a.n2, kStatsBlocks2);
  const dim3 grid(a.blocks2 + (a.n1 > 0 ? blocks(a.n1, kStatsBlocks1) : 0)), block(256);
  if (dim == 3) {
    if (scalar) hipLaunchKernelGGL((k_stats_update<3, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_stats_update<3, false>), grid, block, 0, s, a);
  } else {
    if (scalar) hipLaunchKernelGGL((k_stats_update<2, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_stats_update<2, false>), grid, block, 0, s, a);
  }
  NSFEM_HIP(hipGetLastError());
}

// One workgroup per group g.  Pass 1: A = sum a_n, sum a_n m_n and the within-node part sum a_n C_n / W; pass 2, with
// the group means known: the between-node part sum a_n (m_n - m_g)(m_n - m_g)^T.  out[g][q], q as the accumulators.
template <int DIM, bool SCALAR>
__global__ __launch_bounds__(256) void k_stats_profile(const double* __restrict__ acc, size_t stride, double inv_w,
                                                       const int32_t* __restrict__ group_ptr,
                                                       const int32_t* __restrict__ nodes,
                                                       const double* __restrict__ weights, double* __restrict__ out) {
  using L = StatsCols<DIM, SCALAR>;
  constexpr int NQ = L::NQ, NV = L::NV, NM = L::NM;
  __shared__ double sh[4 * (NQ + 1)];
  const int g = (int)blockIdx.x;
  const int k0 = group_ptr[g], k1 = group_ptr[g + 1];
  double s1[NQ + 1];   // columns, then A
#pragma unroll
  for (int j = 0; j <= NQ; ++j) s1[j] = 0.0;
  for (int k = k0 + (int)threadIdx.x; k < k1; k += 256) {
    const size_t n = (size_t)nodes[k];
    const double a = weights[k];
    s1[NQ] += a;
#pragma unroll
    for (int c = 0; c < NQ; ++c) s1[c] += a * acc[(size_t)c * stride + n];
  }
  block_sum_all<NQ + 1>(s1, sh);
  const double inv_a = 1.0 / s1[NQ];
  double mg[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) mg[v] = s1[L::mean(v)] * inv_a;
  double s2[NM];   // the second-moment columns, counted as stats_for_each_pair counts them
#pragma unroll
  for (int j = 0; j < NM; ++j) s2[j] = 0.0;
  for (int k = k0 + (int)threadIdx.x; k < k1; k += 256) {
    const size_t n = (size_t)nodes[k];
    const double a = weights[k];
    double d[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) d[v] = acc[(size_t)L::mean(v) * stride + n] - mg[v];
    stats_for_each_pair<DIM, SCALAR>([&](int, int k, int i, int j) { s2[k] += a * (d[i] * d[j]); });
  }
  block_sum_all<NM>(s2, sh);
  if (threadIdx.x == 0) {
    double* o = out + (size_t)g * NQ;
#pragma unroll
    for (int v = 0; v < NV; ++v) o[L::mean(v)] = mg[v];
    stats_for_each_pair<DIM, SCALAR>([&](int c, int k, int, int) { o[c] = (s1[c] * inv_w + s2[k]) * inv_a; });
  }
}

void launch_stats_profile(hipStream_t s, int dim, bool scalar, const double* acc, size_t stride, double inv_w,
                          int32_t n_groups, const int32_t* group_ptr, const int32_t* nodes, const double* weights,
                          double* out) {
  if (n_groups <= 0) return;
  const dim3 grid(n_groups), block(256);
#define NSFEM_STATS_PROFILE(D, S) \
  hipLaunchKernelGGL((k_stats_profile<D, S>), grid, block, 0, s, acc, stride, inv_w, group_ptr, nodes, weights, out)
  if (dim == 1) NSFEM_STATS_PROFILE(1, false);
  else if (dim == 2 && !scalar) NSFEM_STATS_PROFILE(2, false);
  else if (dim == 2) NSFEM_STATS_PROFILE(2, true);
  else if (!scalar) NSFEM_STATS_PROFILE(3, false);
  else NSFEM_STATS_PROFILE(3, true);
#undef NSFEM_STATS_PROFILE
  NSFEM_HIP(hipGetLastError());
}

// nc >= 1: out[node][c] = scale * column (col + c); nc = 0: out[node] = scale * (sum of the columns tr[0 .. dim))
__global__ __launch_bounds__(256) void k_stats_gather(int64_t n, const double* __restrict__ acc, size_t stride, int col,
                                                      int nc, double scale, int dim, int tr0, int tr1, int tr2,
                                                      double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (nc == 0) {
      double t = acc[(size_t)tr0 * stride + i];
      if (dim > 1) t += acc[(size_t)tr1 * stride + i];
      if (dim > 2) t += acc[(size_t)tr2 * stride + i];
      out[i] = scale * t;
    } else {
      for (int c = 0; c < nc; ++c) out[(size_t)i * nc + c] = scale * acc[(size_t)(col + c) * stride + i];
    }
  }
}

void launch_stats_gather(hipStream_t s, int64_t n, const double* acc, size_t stride, int col, int nc, double scale,
                         int dim, const int col_trace[3], double* out) {
  if (n <= 0) return;
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(k_stats_gather, dim3(grid), dim3(256), 0, s, n, acc, stride, col, nc, scale, dim, col_trace[0],
                     col_trace[1], col_trace[2], out);
  NSFEM_HIP(hipGetLastError());
}

}  // namespace nsfem
