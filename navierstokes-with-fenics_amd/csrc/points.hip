// Point location, point evaluation and passive tracer particles on the device.
//
// The reference evaluates a dolfin.Function at a point through the bounding-box tree of the mesh (u(x), p(x) in the
// post-processing of its demos: demo/dfg_benchmark.py pressure difference, centre-line profiles); the host path of this
// repository (fem_spaces.evaluate_lagrange) solves a dim x dim system for every cell of the mesh per point.  Here the
// host lays a uniform grid of bins over the mesh once (point_locator.build_bins: per bin the cells whose inflated
// bounding box overlaps it, ascending cell id) and the device searches:
//
//   k_locate_points<DIM>   one thread per point: bin of the point, candidates in list order, first cell whose DIM + 1
//                          barycentric coordinates are all >= -1e-12 (the rule and the tolerance of evaluate_lagrange,
//                          which takes the lowest such cell id); -1 outside the mesh
//   k_eval_points<DIM>     one thread per point, the cell given: P2 / P1 basis from the barycentric coordinates, nodal
//                          values gathered through the dof maps; NaN where the cell is -1
//   k_advect_tracers<DIM>  one thread per particle: classical RK4 over n_sub substeps in the velocity field blended
//                          linearly in time between two state slots; every stage point is located, the last known cell
//                          first and the bins only when the point has left it
//
// Plain loads and stores, no atomics, no floating point reduction: the same input gives the same bytes.  The two
// counters of the tracer kernels (particles that have left, bin-search fallbacks) are integer sums per workgroup, added
// on the host.
#include "cell_geometry.hpp"
#include "element_front.hpp"

namespace nsfem {

namespace {

constexpr double kInsideTol = -1e-12;

// barycentric coordinates of x in cell c: lam[0] = 1 - sum of the reference coordinates J^-1 (x - x_0)
template <int DIM>
__device__ __forceinline__ void barycentric(const double* __restrict__ vx, int nc, int c, const double* x,
                                            double* lam) {
  if constexpr (DIM == 2) {
    const CellGeo g = load_geo(vx, nc, c);
    const double dx = x[0] - vx[c], dy = x[1] - vx[(size_t)nc + c];
    lam[1] = g.ji00 * dx + g.ji01 * dy;
    lam[2] = g.ji10 * dx + g.ji11 * dy;
    lam[0] = 1.0 - (lam[1] + lam[2]);
  } else {
    const CellGeo3 g = load_geo3(vx, nc, c);
    double d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = x[a] - vx[(size_t)a * nc + c];
#pragma unroll
    for (int b = 0; b < 3; ++b) lam[b + 1] = g.ji[b][0] * d[0] + g.ji[b][1] * d[1] + g.ji[b][2] * d[2];
    lam[0] = 1.0 - ((lam[1] + lam[2]) + lam[3]);
  }
}

template <int DIM>
__device__ __forceinline__ bool inside(const double* lam) {
  bool in = true;
#pragma unroll
  for (int i = 0; i <= DIM; ++i) in = in && lam[i] >= kInsideTol;   // false for NaN
  return in;
}

// first candidate of the point's bin that contains it (-1: none); lam holds its barycentric coordinates
template <int DIM>
__device__ __forceinline__ int bin_search(const PointLocatorDev& L, const double* __restrict__ vx, int nc,
                                          const double* x, double* lam) {
  int64_t bin = 0, stride = 1;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const double t = (x[d] - L.origin[d]) * L.inv_h[d];
    if (!(t >= 0.0 && t < (double)L.nbins[d])) return -1;   // outside the grid of bins, or NaN
    bin += stride * (int64_t)t;
    stride *= L.nbins[d];
  }
  const int32_t b0 = L.bin_ptr[bin], b1 = L.bin_ptr[bin + 1];
  for (int32_t k = b0; k < b1; ++k) {
    const int c = L.bin_cells[k];
    barycentric<DIM>(vx, nc, c, x, lam);
    if (inside<DIM>(lam)) return c;
  }
  return -1;
}

// sum_k N_k u[node_k] of a node-interleaved P2 field with NV components
template <int DIM, int NV>
__device__ __forceinline__ void p2_gather(const int32_t* __restrict__ p2, int nc, int c, const double* N,
                                          const double* __restrict__ u, double* out) {
  constexpr int N2 = DIM == 2 ? 6 : 10;
#pragma unroll
  for (int a = 0; a < NV; ++a) out[a] = 0.0;
#pragma unroll
  for (int k = 0; k < N2; ++k) {
    double v[NV];
    load_node<NV, true>(u, (size_t)p2[(size_t)k * nc + c], v);
#pragma unroll
    for (int a = 0; a < NV; ++a) out[a] += N[k] * v[a];
  }
}

}  // namespace

template <int DIM>
__global__ __launch_bounds__(256) void k_locate_points(PointLocatorDev L, int nc, const double* __restrict__ vx,
                                                       int64_t n, const double* __restrict__ x,
                                                       int32_t* __restrict__ cells) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p[DIM], lam[DIM + 1];
#pragma unroll
  for (int d = 0; d < DIM; ++d) p[d] = x[DIM * i + d];
  cells[i] = bin_search<DIM>(L, vx, nc, p, lam);
}

// kind 0: velocity (DIM components, out [n][DIM]), 1: P1 pressure, 2: P2 scalar (out [n])
template <int DIM>
__global__ __launch_bounds__(256) void k_eval_points(int kind, int nc, const double* __restrict__ vx,
                                                     const int32_t* __restrict__ p2, const int32_t* __restrict__ p1,
                                                     const double* __restrict__ f, int64_t n,
                                                     const double* __restrict__ x, const int32_t* __restrict__ cells,
                                                     double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = cells[i];
  const int nv = kind == 0 ? DIM : 1;
  if (c < 0 || c >= nc) {
    for (int a = 0; a < nv; ++a) out[nv * i + a] = __builtin_nan("");
    return;
  }
  double p[DIM], lam[DIM + 1];
#pragma unroll
  for (int d = 0; d < DIM; ++d) p[d] = x[DIM * i + d];
  barycentric<DIM>(vx, nc, c, p, lam);
  if (kind == 1) {
    double v = 0.0, fn[DIM + 1];
    gather_p1<DIM>(p1, nc, c, f, nullptr, fn);
#pragma unroll
    for (int k = 0; k <= DIM; ++k) v += lam[k] * fn[k];
    out[i] = v;
    return;
  }
  double N[DIM == 2 ? 6 : 10];
  p2_at<DIM>(lam, N);   // (the local numbering of evaluate_lagrange)
  if (kind == 0) {
    double v[DIM];
    p2_gather<DIM, DIM>(p2, nc, c, N, f, v);
#pragma unroll
    for (int a = 0; a < DIM; ++a) out[DIM * i + a] = v[a];
  } else {
    double v[1];
    p2_gather<DIM, 1>(p2, nc, c, N, f, v);
    out[i] = v[0];
  }
}

// status of freshly located particles (cell -1: left) and the number of them per workgroup
__global__ __launch_bounds__(256) void k_tracer_init(int64_t n, const int32_t* __restrict__ cells,
                                                     uint8_t* __restrict__ status, int32_t* __restrict__ counts) {
  __shared__ int sh[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int left = 0;
  if (i < n) {
    left = cells[i] < 0 ? 1 : 0;
    status[i] = (uint8_t)left;
  }
  const int sum[1] = {left};
  block_sum_fixed<1>(sum, sh);
  if (threadIdx.x == 0) {
    counts[2 * blockIdx.x] = block_total<1>(sh, 0);
    counts[2 * blockIdx.x + 1] = 0;
  }
}

// u(p, theta) = (1 - theta) ua + theta ub in a cell that contains p (ub null: the frozen field ua); false when p lies
// outside the mesh.  `cell` is tested first and replaced by the cell found.
template <int DIM>
__device__ __forceinline__ bool tracer_velocity(const PointLocatorDev& L, int nc, const double* __restrict__ vx,
                                                const int32_t* __restrict__ p2, const double* __restrict__ ua,
                                                const double* __restrict__ ub, double theta, const double* p,
                                                int& cell, int& fallbacks, double* vel) {
  double lam[DIM + 1];
  barycentric<DIM>(vx, nc, cell, p, lam);
  if (!inside<DIM>(lam)) {
    ++fallbacks;
    const int c = bin_search<DIM>(L, vx, nc, p, lam);
    if (c < 0) return false;
    cell = c;
  }
  double N[DIM == 2 ? 6 : 10];
  p2_at<DIM>(lam, N);   // (the local numbering of evaluate_lagrange)
  p2_gather<DIM, DIM>(p2, nc, cell, N, ua, vel);
  if (ub) {
    double vb[DIM];
    p2_gather<DIM, DIM>(p2, nc, cell, N, ub, vb);
#pragma unroll
    for (int a = 0; a < DIM; ++a) vel[a] = (1.0 - theta) * vel[a] + theta * vb[a];
  }
  return true;
}

// counts[2 b] = particles of workgroup b with status != 0 after the call, counts[2 b + 1] = its bin-search fallbacks
template <int DIM>
__global__ __launch_bounds__(256) void k_advect_tracers(PointLocatorDev L, int nc, const double* __restrict__ vx,
                                                        const int32_t* __restrict__ p2,
                                                        const double* __restrict__ ua, const double* __restrict__ ub,
                                                        double dt, int n_sub, int64_t n, double* __restrict__ x,
                                                        int32_t* __restrict__ cells, uint8_t* __restrict__ status,
                                                        int32_t* __restrict__ counts) {
  __shared__ int sh[4 * 2];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int left = 0, fallbacks = 0;
  if (i < n) left = status[i] != 0 ? 1 : 0;
  if (i < n && !left) {
    double x0[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) x0[d] = x[DIM * i + d];
    int cell = cells[i];
    const double h = dt / (double)n_sub;
    for (int s = 0; s < n_sub; ++s) {
      const double th0 = (double)s / (double)n_sub, th1 = ((double)s + 0.5) / (double)n_sub,
                   th2 = (double)(s + 1) / (double)n_sub;
      double k1[DIM], k2[DIM], k3[DIM], k4[DIM], p[DIM];
      int c = cell;
      bool ok = tracer_velocity<DIM>(L, nc, vx, p2, ua, ub, th0, x0, c, fallbacks, k1);
      if (ok) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) p[d] = x0[d] + 0.5 * h * k1[d];
        ok = tracer_velocity<DIM>(L, nc, vx, p2, ua, ub, th1, p, c, fallbacks, k2);
      }
      if (ok) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) p[d] = x0[d] + 0.5 * h * k2[d];
        ok = tracer_velocity<DIM>(L, nc, vx, p2, ua, ub, th1, p, c, fallbacks, k3);
      }
      if (ok) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) p[d] = x0[d] + h * k3[d];
        ok = tracer_velocity<DIM>(L, nc, vx, p2, ua, ub, th2, p, c, fallbacks, k4);
      }
      if (ok) {
        // the end point of a substep is the first stage point of the next one; it is located here, so that the
        // cell kept with the particle contains the position kept with it after the last substep as well
        double lam[DIM + 1];
#pragma unroll
        for (int d = 0; d < DIM; ++d) p[d] = x0[d] + (h / 6.0) * ((k1[d] + 2.0 * k2[d]) + (2.0 * k3[d] + k4[d]));
        barycentric<DIM>(vx, nc, c, p, lam);
        if (!inside<DIM>(lam)) {
          ++fallbacks;
          c = bin_search<DIM>(L, vx, nc, p, lam);
          ok = c >= 0;
        }
      }
      if (!ok) {
        left = 1;
        break;
      }
#pragma unroll
      for (int d = 0; d < DIM; ++d) x0[d] = p[d];
      cell = c;
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) x[DIM * i + d] = x0[d];
    cells[i] = cell;
    if (left) status[i] = 1;
  }
  const int sum[2] = {left, fallbacks};
  block_sum_fixed<2>(sum, sh);
  store_block_partials<2>(sh, counts, 2 * blockIdx.x, 1, 0);
}

static inline unsigned point_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

void launch_locate_points(hipStream_t s, const MeshDev& m, const PointLocatorDev& L, int64_t n, const double* x,
                          int32_t* cells) {
  if (n == 0) return;
  if (m.dim == 3)
    hipLaunchKernelGGL(k_locate_points<3>, dim3(point_blocks(n)), dim3(256), 0, s, L, m.n_cells, m.vx.p, n, x, cells);
  else
    hipLaunchKernelGGL(k_locate_points<2>, dim3(point_blocks(n)), dim3(256), 0, s, L, m.n_cells, m.vx.p, n, x, cells);
  NSFEM_HIP(hipGetLastError());
}

void launch_eval_points(hipStream_t s, const MeshDev& m, int kind, const double* f, int64_t n, const double* x,
                        const int32_t* cells, double* out) {
  if (n == 0) return;
  if (m.dim == 3)
    hipLaunchKernelGGL(k_eval_points<3>, dim3(point_blocks(n)), dim3(256), 0, s, kind, m.n_cells, m.vx.p, m.p2.p,
                       m.p1.p, f, n, x, cells, out);
  else
    hipLaunchKernelGGL(k_eval_points<2>, dim3(point_blocks(n)), dim3(256), 0, s, kind, m.n_cells, m.vx.p, m.p2.p,
                       m.p1.p, f, n, x, cells, out);
  NSFEM_HIP(hipGetLastError());
}

void launch_tracer_init(hipStream_t s, int64_t n, const int32_t* cells, uint8_t* status, int32_t* counts) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_tracer_init, dim3(point_blocks(n)), dim3(256), 0, s, n, cells, status, counts);
  NSFEM_HIP(hipGetLastError());
}

void launch_advect_tracers(hipStream_t s, const MeshDev& m, const PointLocatorDev& L, const double* ua,
                           const double* ub, double dt, int n_sub, int64_t n, double* x, int32_t* cells,
                           uint8_t* status, int32_t* counts) {
  if (n == 0) return;
  if (m.dim == 3)
    hipLaunchKernelGGL(k_advect_tracers<3>, dim3(point_blocks(n)), dim3(256), 0, s, L, m.n_cells, m.vx.p, m.p2.p, ua,
                       ub, dt, n_sub, n, x, cells, status, counts);
  else
    hipLaunchKernelGGL(k_advect_tracers<2>, dim3(point_blocks(n)), dim3(256), 0, s, L, m.n_cells, m.vx.p, m.p2.p, ua,
                       ub, dt, n_sub, n, x, cells, status, counts);
  NSFEM_HIP(hipGetLastError());
}

}  // namespace nsfem
